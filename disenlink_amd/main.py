"""Command-line driver with the flags of the reference's ``main_disentangled.py`` (:21-50), running the
pair-list pipeline on the MI355X path:

    python -m disenlink_amd.main --dataset chameleon --beta 0.7 --nfactor 5 --nhidden 512 --nembed 32 \\
        --epochs 2000 --lr 0.0001 --m 5 --run 10 [--data-root /path/to/reference/data | --data-file ds.npz]

Differences from the reference script, on purpose: runs are seeded (``--seed`` + run index; the reference
seeds nothing on the CPU path, SURVEY.md §0 finding 5); the split / masks / loss / AUC work on pair lists
(no ``[N,N]`` tensors); flags the reference parses but never uses (``--weight_decay``, ``--nfeat``,
``--loss_weight``, ``--debug``, ``--layer`` other than 1) are accepted and ignored the same way.
Without data files a seeded synthetic stand-in of the named dataset is used (``disenlink_amd.data``).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--debug", action="store_true", default=False)
    p.add_argument("--no-cuda", action="store_true", default=False)
    p.add_argument("--seed", type=int, default=18)
    p.add_argument("--lr", type=float, default=0.0001)
    p.add_argument("--beta", type=float, default=0.9)
    p.add_argument("--nfactor", type=int, default=3)
    p.add_argument("--weight_decay", type=float, default=5e-4)
    p.add_argument("--nfeat", type=int, default=128)
    p.add_argument("--nhidden", type=int, default=512)
    p.add_argument("--nembed", type=int, default=32)
    p.add_argument("--epochs", type=int, default=2000)
    p.add_argument("--temperature", type=int, default=1)
    p.add_argument("--dataset", type=str, default="chameleon")
    p.add_argument("--sub_dataset", type=str, default="Amherst41")
    p.add_argument("--run", type=int, default=10)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--m", type=int, default=5)
    p.add_argument("--save", type=int, default=0)
    p.add_argument("--loss_weight", type=int, default=20)
    p.add_argument("--layer", type=int, default=1)
    p.add_argument("--miniid", type=int, default=9)
    # extensions
    p.add_argument("--data-root", type=str, default=None, help="directory laid out like the reference's data/")
    p.add_argument("--data-file", type=str, default=None, help="binary dataset written by datasets.save_binary")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic stand-in of --dataset")
    p.add_argument("--table-dtype", choices=["f32", "bf16"], default="f32")
    p.add_argument("--resample-negatives", action="store_true",
                   help="with --objective pairs / pairs-logit: draw the training negatives anew every epoch on the device "
                        "(m per training edge row, never an edge row of the dataset; duplicates kept) instead of training on "
                        "the split's fixed sample; one GPU, eager loop, fp32 tables")
    p.add_argument("--resample-seed", type=int, default=0, help="seed of --resample-negatives (the draw is a pure function of "
                                                                "seed, epoch and entry)")
    p.add_argument("--hard-negatives", type=int, default=0, metavar="C",
                   help="with --resample-negatives or --objective bpr: hard negatives — every epoch draw C candidates per entry "
                        "(2 <= C <= 64) and keep the one the current model scores highest (dynamic negative sampling, on the "
                        "device, no plan build); 0 or 1: the plain uniform draw.  Biased towards false negatives on graphs with "
                        "many unobserved true links")
    p.add_argument("--objective", choices=["pairs", "pairs-logit", "recon", "recon-logit", "bpr"], default="pairs",
                   help="the training loss: bpr = the pairwise ranking loss, every training edge (u, v) must score above (u, k) "
                        "for m negatives k drawn anew every epoch on the device (softplus of the logit difference; implies "
                        "--resample-negatives, --resample-seed applies; AUC counted on logits; one GPU, eager loop, fp32 "
                        "tables); pairs = the reference's BCE on m sampled negatives per edge; pairs-logit = the same "
                        "pairs with the BCE taken of the LOGITS (a saturated pair keeps its gradient, and the validation / test "
                        "AUC is counted on logits, which do not tie at probability 1; one GPU); recon = the "
                        "whole-graph reconstruction loss, every non-edge a negative and the edges up-weighted, with the "
                        "validation and test pairs ignored (Disentangle.forward_recon_loss: nothing of size N x N is formed; "
                        "one GPU, eager loop; with --table-dtype bf16 it runs on the bf16 tables the model is evaluated on); "
                        "recon-logit = recon with the loss taken of the LOGITS (Disentangle.forward_recon_logits_loss: a non-edge "
                        "the model scores past the saturation of the fp32 sigmoid keeps its cost and its gradient; AUC counted "
                        "on logits; --pos-weight, --recon-block-rows and --table-dtype apply as for recon)")
    p.add_argument("--pos-weight", type=float, default=None,
                   help="with --objective recon / recon-logit: the weight of a positive pair (default: negatives / positives)")
    p.add_argument("--recon-block-rows", type=int, default=None,
                   help="with --objective recon / recon-logit: rows per strip, a multiple of 128 (default: the largest strip of at most 1 GiB)")
    p.add_argument("--no-graph", action="store_true",
                   help="launch every epoch from Python instead of replaying it from a captured HIP graph")
    p.add_argument("--graph", action="store_true",
                   help="replay every epoch from a captured HIP graph.  Default: replayed when the compiled binding "
                        "(libdisenlink_torch.so) is absent, eager when it is present — with it and the end-of-epoch "
                        "bookkeeping on the device the eager loop is gapless and 3-10 %% faster than the replay")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--scan-dtype", choices=["f32", "bf16"], default="f32",
                   help="tables of the all-pairs scans (--rank-eval, --global-rank-eval, --mine, --predict-links, --predict-top): f32, "
                        "or "
                        "bf16 = Z rounded to bf16 and H aggregated from it, as the bf16 training step forms them; one "
                        "matrix-core product per block instead of six and a third of the plane workspace")
    p.add_argument("--rank-eval", action="store_true",
                   help="after each run, rank every test positive among all nodes (filtered by every dataset edge) and "
                        "print MRR and Hits@{1,10,50,100}")
    p.add_argument("--global-rank-eval", action="store_true",
                   help="after each run, rank every test positive among ALL unordered pairs of the graph (filtered by every "
                        "dataset edge) and print the AUC against every non-edge, mean rank, MRR and recall@{100,1000,10000} "
                        "(Disentangle.missing_link_ranks; single GPU, fp32 tables)")
    p.add_argument("--mine", type=int, default=0, metavar="M",
                   help="after the last run, list the M (<= 65536) most likely links of the whole graph that are not dataset "
                        "edges (Disentangle.top_missing_links; single GPU, fp32 tables; graphs of more than 46340 nodes are "
                        "scanned by blocks of 46208)")
    p.add_argument("--mine-out", type=str, default=None, metavar="FILE",
                   help="with --mine: write the list to FILE as text, one `src dst logit prob` line per pair")
    p.add_argument("--predict-links", type=float, default=None, metavar="P",
                   help="after the last run, form the predicted graph: every pair that is not a dataset edge and whose "
                        "link_pred reaches P (Disentangle.predicted_links; single GPU, fp32 tables; graphs of more than 46340 "
                        "nodes are scanned by blocks of 46208), and print "
                        "the number of links, the density and the mean / max predicted degree")
    p.add_argument("--predict-top", type=int, default=None, metavar="M",
                   help="after the last run, form the predicted graph under a budget: the M most likely pairs that are not "
                        "dataset edges, for any M >= 1 (Disentangle.top_predicted_links; single GPU, fp32 tables, "
                        "N <= 46340), printed as --predict-links prints its links; not together with --predict-links")
    p.add_argument("--links-out", type=str, default=None, metavar="FILE",
                   help="with --predict-links / --predict-top: write the links to FILE as text, one `src dst prob` line per pair, src < dst")
    p.add_argument("--explain", action="store_true",
                   help="with --mine / --predict-links / --predict-top: say which of the K factors makes each listed link "
                        "(Disentangle.explain_links: the per-factor terms of the scans' own pass).  --mine-out lines gain "
                        "`factor contrib[factor]`, --links-out lines gain `factor`, and the number of links per dominant "
                        "factor is printed")
    p.add_argument("--node-groups", type=str, default=None, metavar="FILE",
                   help="with --link-rule: the group (an integer in 0..63) of every node, one per node, as text or .npy")
    p.add_argument("--link-rule", choices=["same", "different"], default=None,
                   help="with --node-groups: --rank-eval, --global-rank-eval, --mine and --predict-links take as candidates "
                        "only links between nodes of the same / of different groups (ops.NodeFilter)")
    p.add_argument("--recon-link-rule", action="store_true",
                   help="with --objective recon / recon-logit and --node-groups / --link-rule: the objective itself takes only "
                        "pairs the rule admits (a denied pair, edge or not, carries no loss and is not counted; the default "
                        "--pos-weight is that of the admitted pairs), so training charges what the filtered evaluation considers")
    p.add_argument("--sparse-features", action="store_true",
                   help="hand the features to the model as features.SparseFeatures (scale * X + shift with X a CSR): layer 1 "
                        "of the projection and its gradient run as gathers over the non-zero entries; for binary / one-hot "
                        "features, standardised or not (single GPU)")
    p.add_argument("--gpus", type=int, default=1,
                   help="row-shard every run over this many GPUs of the node (one process per GPU, RCCL): started "
                        "plainly, the command launches its ranks itself (disenlink_amd/launch.py)")
    return p


_STANDARDISING_LOADERS = ("load_npz", "load_fb100", "load_twitch", "load_webkb", "load_amazon_npz", "load_deezer",
                          "load_arxiv_year_mini")


def load_dataset(args, raw: bool = False):
    """The dataset of the command line.  raw=True (--sparse-features): -> (dataset with UNstandardised features, whether
    the loader would have standardised their rows) — features.SparseFeatures.from_dense applies the standardisation as its
    per-row scale and shift."""
    from . import datasets
    if not raw:
        return _load_dataset(args, datasets)

    class _Raw:                                                      # the loaders that standardise, asked not to
        def __init__(self):
            self.standardised = False

        def __getattr__(self, name):
            fn = getattr(datasets, name)
            if name not in _STANDARDISING_LOADERS:
                return fn

            def call(*a, **kw):
                self.standardised = True
                return fn(*a, standardise=False, **kw)
            return call
    shim = _Raw()
    ds = _load_dataset(args, shim)
    return ds, shim.standardised


def _load_dataset(args, datasets):
    from .data import SPECS, synthetic_graph
    if args.data_file:
        return datasets.load_binary(args.data_file)
    root = args.data_root
    if root and not args.synthetic:
        name = args.dataset
        if name in ("chameleon", "squirrel", "crocodile"):          # main_disentangled.py:73-81, 97-108
            npz = os.path.join(os.path.dirname(root.rstrip("/")), "data_pre_false", name, "raw", f"{name}.npz")
            if not os.path.exists(npz):
                npz = os.path.join(root, name, "raw", f"{name}.npz")
            return datasets.load_npz(npz, name)
        if name in ("cora", "citeseer", "pubmed"):                  # :117-123
            return datasets.load_planetoid(os.path.join(root, name, "raw"), name)
        if name == "fb100":                                         # :62-64, 109-113
            return datasets.load_fb100(os.path.join(root, "facebook100", args.sub_dataset + ".mat"), args.sub_dataset)
        if name == "twitch-e":                                      # :62-64, 109-116
            return datasets.load_twitch(os.path.join(root, "twitch", args.sub_dataset), args.sub_dataset)
        if name in ("texas", "wisconsin", "cornell"):               # :69-71, 91-96
            return datasets.load_webkb(os.path.join(root, name, "raw"), name)
        if name == "photo":                                         # :66-68, 85-90
            return datasets.load_amazon_npz(os.path.join(root, "Photo", "raw", "amazon_electronics_photo.npz"))
        if name == "deezer-europe":                                 # :58-59, 109-113
            return datasets.load_deezer(os.path.join(root, "deezer-europe.mat"))
        if name == "year":                                          # :124-129 (the arxiv-year minis, --miniid 0..9)
            return datasets.load_arxiv_year_mini(os.path.join(os.path.dirname(root.rstrip("/")), "mini", f"year{args.miniid}.pt"),
                                                 f"year{args.miniid}")
        raise SystemExit(f"no loader for --dataset {name} (ogbn-proteins / the full arxiv-year / yelp-chi need the ogb "
                         f"download layout: convert with datasets.save_binary and pass --data-file)")
    key = {"fb100": "penn94", "snap-patents": "snap_patents"}.get(args.dataset, args.dataset)
    if key not in SPECS:
        raise SystemExit(f"no data for --dataset {args.dataset}: give --data-root / --data-file")
    sg = synthetic_graph(key, seed=args.seed)
    return datasets.LinkDataset(f"{key}-synthetic", sg.features(), sg.src, sg.dst)


def save_results(args, result) -> None:
    """--save 1: append the runs' summary line to performance/<dataset>_..._nfactor.csv (main_disentangled.py:225-246)."""
    os.makedirs("performance", exist_ok=True)
    sub = f"{args.sub_dataset}" if args.dataset in ("twitch-e", "fb100") else ""
    with open(f"performance/{args.dataset}_{sub}disentangle_nfactor.csv", "a+") as f:
        f.write(f"{result.mean():.3f} ± {result.std():.3f},{result},beta {args.beta},temperature {args.temperature},"
                f"nfactor {args.nfactor},nhidden {args.nhidden},nembed {args.nembed},dataset {args.dataset},"
                f"run {args.run},epochs {args.epochs},lr {args.lr},m {args.m}\n")


def main_sharded(args):
    """--gpus N: the same runs with the graph's rows, the feature rows and the pair lists sharded over N ranks
    (train.run_link_prediction_sharded).  Every rank loads the dataset and draws the SAME seeded split (host arrays);
    it keeps its own feature rows only.  Rank 0 prints."""
    import torch.distributed as dist
    from .model import Disentangle
    from .splits import make_link_split
    from .train import prepare_run_sharded, run_link_prediction_sharded
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    rehearse = bool(os.environ.get("DL_REHEARSE_ON_ONE_GPU"))      # all ranks on cuda:0, gloo collectives: functional only
    device = torch.device("cuda", 0 if rehearse else local)
    torch.cuda.set_device(device)
    if rehearse:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    say = (lambda *a: print(*a, flush=True)) if rank == 0 and not args.quiet else (lambda *a: None)
    try:
        ds = load_dataset(args)
        say(args)
        say(f"dataset {ds.name}: N={ds.n_nodes} F={ds.x.shape[1]} edge rows={ds.src.size}; row-sharded over {world} GPUs")
        tdt = torch.bfloat16 if args.table_dtype == "bf16" else torch.float32
        row_bytes = args.nfactor * args.nembed * (2 if args.table_dtype == "bf16" else 4)
        result = []
        for run in range(args.run):
            say("run:", run)
            split = make_link_split(ds.src, ds.dst, ds.n_nodes, m=args.m, seed=args.seed + run)
            prepared = prepare_run_sharded(split, rank, world, device, row_bytes=row_bytes)
            r0, r1 = prepared.shard.local_real_rows()
            x_loc = torch.from_numpy(np.ascontiguousarray(ds.x[r0:r1])).to(device)
            torch.manual_seed(args.seed + run)                       # identical replicas
            model = Disentangle(ds.x.shape[1], args.nhidden, args.nembed, nfactor=args.nfactor, beta=args.beta,
                                t=args.temperature, table_dtype=tdt).to(device)
            res = run_link_prediction_sharded(model, x_loc, prepared, epochs=args.epochs, lr=args.lr,
                                              log=say if not args.quiet else None)
            say("test auc:", res.test_auc)
            result.append(res.test_auc)
        result = np.array(result)
        if rank == 0:
            print("final", result.mean(), result.std(), flush=True)
            if args.save == 1:
                save_results(args, result)
        return result
    finally:
        dist.destroy_process_group()


def load_node_groups(path: str, n_nodes: int, rule: str, device):
    """--node-groups FILE --link-rule RULE as an ops.NodeFilter on ``device``."""
    from .ops import NodeFilter
    try:
        g = np.load(path, allow_pickle=False) if path.endswith(".npy") else np.loadtxt(path, dtype=np.int64, ndmin=1)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--node-groups {path}: {e}")
    g = np.asarray(g)
    if g.ndim != 1 or g.size != n_nodes or not np.issubdtype(g.dtype, np.integer):
        raise SystemExit(f"--node-groups {path}: expected one integer per node ({n_nodes}), got shape {g.shape} {g.dtype}")
    if g.size and (g.min() < 0 or g.max() > 63):
        raise SystemExit(f"--node-groups {path}: groups outside 0..63")
    make = NodeFilter.same if rule == "same" else NodeFilter.different
    return make(torch.from_numpy(g.astype(np.int64)), device=device)


def scan_table_dtype(args):
    """--scan-dtype as the ``table_dtype`` keyword of the Disentangle scan methods (None = fp32 tables)."""
    return torch.bfloat16 if args.scan_dtype == "bf16" else None


def rank_eval(model, x, graph, split, known, node_filter=None, table_dtype=None) -> dict:
    """MRR and Hits@{1,10,50,100} of the test positives, each ranked among all nodes with every known edge filtered out
    (Disentangle.link_ranks: the model with its best weights, as run_link_prediction leaves it)."""
    from .metrics import ranking_metrics
    pos = split.test.label > 0.5
    src = torch.from_numpy(np.ascontiguousarray(split.test.u[pos])).to(x.device)
    dst = torch.from_numpy(np.ascontiguousarray(split.test.v[pos])).to(x.device)
    greater, ties = model.link_ranks(x, graph, src, dst, exclude=known, node_filter=node_filter, table_dtype=table_dtype)
    return ranking_metrics(greater, ties)


def global_rank_eval(model, x, graph, split, known, node_filter=None, table_dtype=None) -> dict:
    """AUC against every non-edge, mean rank, MRR and recall@M of the test positives, each ranked among all unordered
    pairs of the graph with every known edge filtered out (Disentangle.missing_link_ranks, the model's best weights);
    self loops among the positives are left out."""
    from .metrics import global_ranking_metrics
    pos = split.test.label > 0.5
    src = torch.from_numpy(np.ascontiguousarray(split.test.u[pos])).to(x.device)
    dst = torch.from_numpy(np.ascontiguousarray(split.test.v[pos])).to(x.device)
    keep = src != dst                                               # a self loop of the dataset is no pair of the graph
    r = model.missing_link_ranks(x, graph, src[keep], dst[keep], exclude=known, node_filter=node_filter, table_dtype=table_dtype)
    return global_ranking_metrics(r.greater, r.ties, r.n_others)


def explain(model, x, graph, src, dst, what: str, log=print, table_dtype=None):
    """--explain: the dominant factor of every listed link and its contribution (Disentangle.explain_links) as numpy arrays
    (a link whose terms hold a NaN has factor -1 and contribution NaN), and one line: links per dominant factor."""
    terms = model.explain_links(x, graph, src, dst, table_dtype=table_dtype)
    factor = terms.factor
    top = terms.contrib.gather(1, factor.clamp(min=0)[:, None])[:, 0]
    top = torch.where(factor < 0, torch.full_like(top, float("nan")), top)
    counts = torch.bincount(factor[factor >= 0], minlength=terms.cum.shape[1]).tolist()
    nan = int((factor < 0).sum())
    log(f"{what} links by dominant factor: " + " ".join(f"{k}:{c}" for k, c in enumerate(counts)) +
        (f" nan:{nan}" if nan else ""))
    return factor.cpu().numpy(), top.cpu().numpy()


def mine_links(model, x, graph, known, m: int, out=None, show: int = 10, log=print, node_filter=None, table_dtype=None,
               explained: bool = False):
    """--mine: the m most likely links outside ``known`` (Disentangle.top_missing_links), the first ``show`` printed and,
    with ``out``, all of them written as `src dst logit prob` lines; ``explained`` (--explain): every line, printed or
    written, ends in `factor contrib[factor]`."""
    mined = model.top_missing_links(x, graph, m, exclude=known, node_filter=node_filter, table_dtype=table_dtype)
    src, dst, logit, prob = (v.cpu().numpy() for v in mined)
    more = [""] * src.size
    if explained:
        factor, top = explain(model, x, graph, mined.src, mined.dst, "mined", log, table_dtype)
        more = [f" {f} {c:.9g}" for f, c in zip(factor.tolist(), top.tolist())]
    log(f"mined {src.size} links (of {m} asked for); first {min(show, src.size)}: src dst logit prob"
        f"{' factor contrib' if explained else ''}")
    for i in range(min(show, src.size)):
        log(f"{src[i]} {dst[i]} {logit[i]:.6g} {prob[i]:.6g}{more[i]}")
    if out:
        with open(out, "w") as fh:
            for i in range(src.size):
                fh.write(f"{src[i]} {dst[i]} {logit[i]:.9g} {prob[i]:.9g}{more[i]}\n")
    return mined


def predict_links(model, x, graph, known, min_prob: float, out=None, log=print, node_filter=None, table_dtype=None,
                  explained: bool = False):
    """--predict-links: every link outside ``known`` whose link_pred reaches ``min_prob`` (Disentangle.predicted_links), a
    summary line printed and, with ``out``, all of them written as `src dst prob` lines, src < dst; ``explained``
    (--explain): the lines end in `factor`, each unordered pair explained once."""
    links = model.predicted_links(x, graph, min_prob, exclude=known, node_filter=node_filter, table_dtype=table_dtype)
    return _report_links(model, x, graph, links, f"at prob >= {min_prob:g}", out, log, table_dtype, explained)


def predict_top_links(model, x, graph, known, m: int, out=None, log=print, node_filter=None, table_dtype=None,
                      explained: bool = False):
    """--predict-top: the ``m`` most likely links outside ``known`` (Disentangle.top_predicted_links), printed and written
    exactly as --predict-links prints and writes its links."""
    links = model.top_predicted_links(x, graph, m, exclude=known, node_filter=node_filter, table_dtype=table_dtype)
    return _report_links(model, x, graph, links, f"under a budget of {m}", out, log, table_dtype, explained)


def _report_links(model, x, graph, links, how: str, out, log, table_dtype, explained: bool):
    """What --predict-links and --predict-top share: the summary line of a PredictedLinks, --explain and --links-out."""
    n = links.n_nodes
    pairs = links.pairs()
    src, dst, _, prob = (v.cpu().numpy() for v in pairs)
    deg = links.degree.cpu().numpy()
    density = src.size / (n * (n - 1) / 2) if n > 1 else 0.0
    log(f"predicted {src.size} links {how}: density {density:.6g} mean degree {deg.mean():.6g} "
        f"max degree {int(deg.max())}")
    factor = None
    if explained:
        factor, _ = explain(model, x, graph, pairs[0], pairs[1], "predicted", log, table_dtype)
    if out:
        with open(out, "w") as fh:                                   # millions of lines at a useful threshold: by chunks
            for i in range(0, src.size, 1 << 16):
                rows = zip(src[i:i + (1 << 16)].tolist(), dst[i:i + (1 << 16)].tolist(), prob[i:i + (1 << 16)].tolist())
                if factor is None:
                    fh.write("".join(f"{a} {b} {p:.9g}\n" for a, b, p in rows))
                else:
                    fh.write("".join(f"{a} {b} {p:.9g} {f}\n" for (a, b, p), f in zip(rows, factor[i:i + (1 << 16)].tolist())))
    return links


def _fmt_ranking(r: dict) -> str:
    return " ".join(f"{key} {val:.4f}" for key, val in r.items())


def _use_graph(args) -> bool:
    """--graph / --no-graph, else by what is faster: the replayed epoch saves host time per launch, which only matters when
    the launches go through the Python operators (chameleon 0.38 vs 0.76 ms); through the compiled binding, with early
    stopping on the device (early_stop.py), the host runs ahead of the GPU and the eager loop has neither the replay's
    per-node dispatch cost nor a gap between epochs (squirrel 0.837 vs 0.860 ms, chameleon 0.313 vs 0.331, cora-sized 0.665 vs
    0.707: profiles/r5z_*)."""
    if args.graph or args.no_graph:
        return bool(args.graph)
    from . import native
    return not native.available()


def main(argv=None):
    args = build_parser().parse_known_args(argv)[0]                 # unknown tokens ignored, like :50
    if args.layer != 1:
        raise SystemExit("only --layer 1 exists in the reference (main_disentangled.py:147-148)")
    if args.gpus > 1 and args.sparse_features:
        raise SystemExit("--sparse-features runs on one GPU only (the sharded path takes dense feature rows): drop --gpus")
    if args.gpus > 1 and args.rank_eval:
        raise SystemExit("--rank-eval runs on one GPU only (sharded ranking is not implemented): drop --gpus or --rank-eval")
    if args.global_rank_eval and (args.gpus > 1 or args.table_dtype == "bf16"):
        raise SystemExit("--global-rank-eval runs on one GPU with fp32 tables only (sharded and bf16 global ranking are not "
                         "implemented): drop --gpus / --table-dtype bf16 or --global-rank-eval")
    if args.mine and (args.gpus > 1 or args.table_dtype == "bf16"):
        raise SystemExit("--mine runs on one GPU with fp32 tables only (sharded and bf16 mining are not implemented): drop "
                         "--gpus / --table-dtype bf16 or --mine")
    if args.mine and not 1 <= args.mine <= 65536:
        raise SystemExit("--mine M: 1 <= M <= 65536")
    if args.predict_links is not None and (args.gpus > 1 or args.table_dtype == "bf16"):
        raise SystemExit("--predict-links runs on one GPU with fp32 tables only (sharded and bf16 link graphs are not "
                         "implemented): drop --gpus / --table-dtype bf16 or --predict-links")
    if args.predict_links is not None and not 0.0 <= args.predict_links <= 1.0:
        raise SystemExit("--predict-links P: 0 <= P <= 1")
    if args.predict_top is not None and args.predict_links is not None:
        raise SystemExit("--predict-top M and --predict-links P each form the predicted graph: give one of them")
    if args.predict_top is not None and (args.gpus > 1 or args.table_dtype == "bf16"):
        raise SystemExit("--predict-top runs on one GPU with fp32 tables only (sharded and bf16 link graphs are not "
                         "implemented): drop --gpus / --table-dtype bf16 or --predict-top")
    if args.predict_top is not None and args.predict_top < 1:
        raise SystemExit("--predict-top M: M >= 1")
    if args.links_out and args.predict_links is None and args.predict_top is None:
        raise SystemExit("--links-out FILE goes with --predict-links P")
    if args.explain and not (args.mine or args.predict_links is not None or args.predict_top is not None):
        raise SystemExit("--explain names the factor behind the links of --mine and --predict-links: give one of them")
    if (args.node_groups is None) != (args.link_rule is None):
        raise SystemExit("--node-groups FILE and --link-rule {same,different} go together")
    if args.link_rule and not (args.rank_eval or args.global_rank_eval or args.mine or args.predict_links is not None or
                               args.predict_top is not None or args.recon_link_rule):
        raise SystemExit("--link-rule restricts the candidates of --rank-eval, --global-rank-eval, --mine and --predict-links "
                         "(and, with --recon-link-rule, the pairs of --objective recon / recon-logit): give one of them")
    if args.recon_link_rule and not args.link_rule:
        raise SystemExit("--recon-link-rule puts the rule of --node-groups FILE --link-rule {same,different} on the objective: "
                         "give them")
    if args.recon_link_rule and args.objective not in ("recon", "recon-logit"):
        raise SystemExit("--recon-link-rule restricts the reconstruction loss: give --objective recon or recon-logit")
    if args.objective in ("recon", "recon-logit") and (args.gpus > 1 or args.graph):
        raise SystemExit("--objective recon runs on one GPU in the eager loop only, with fp32 or bf16 tables (sharded and "
                         "graph-replayed reconstruction epochs are not implemented): drop --gpus / --graph")
    if args.objective == "bpr" and (args.gpus > 1 or args.graph or args.table_dtype == "bf16"):
        raise SystemExit("--objective bpr runs on one GPU in the eager loop with fp32 tables (the sharded step, HIP-graph replay "
                         "of a resampled epoch and bf16 tables are not implemented): drop --gpus / --graph / bf16")
    resample = args.resample_negatives or args.objective == "bpr"    # the ranking objective draws its negatives every epoch
    if args.resample_negatives:
        if args.objective not in ("pairs", "pairs-logit", "bpr"):
            raise SystemExit("--resample-negatives goes with --objective pairs or pairs-logit (--objective bpr implies it)")
        if args.gpus > 1 or args.graph or args.table_dtype == "bf16":
            raise SystemExit("--resample-negatives runs on one GPU in the eager loop with fp32 tables (the sharded step, HIP-graph "
                             "replay of a resampled epoch and bf16 tables are not implemented): drop --gpus / --graph / bf16")
    if not 0 <= args.hard_negatives <= 64:
        raise SystemExit(f"--hard-negatives takes 0 .. 64 candidates per entry (one lane draws one candidate), got {args.hard_negatives}")
    if args.hard_negatives and not resample:
        raise SystemExit("--hard-negatives chooses among candidates drawn every epoch: give --resample-negatives (with --objective "
                         "pairs or pairs-logit) or --objective bpr")
    if args.objective == "pairs-logit" and args.gpus > 1:
        raise SystemExit("--objective pairs-logit runs on one GPU only (the sharded step has no logit-space form): drop --gpus")
    if args.gpus > 1:
        from .launch import launch_ranks, under_launcher
        if not under_launcher():                                    # BEFORE any GPU call: the parent starts and waits
            entry = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rank_entry.py")
            import json
            raise SystemExit(launch_ranks(args.gpus, [entry], [], env_extra={
                "DL_MAIN_ARGV": json.dumps(list(sys.argv[1:] if argv is None else argv))}))
        if args.no_cuda or not torch.cuda.is_available():
            raise SystemExit("disenlink_amd runs on the GPU only (libdisenlink_hip.so has no CPU fallback)")
        return main_sharded(args)
    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit("disenlink_amd runs on the GPU only (libdisenlink_hip.so has no CPU fallback)")
    from .model import Disentangle
    from .splits import make_link_split
    from .train import prepare_run, run_link_prediction
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    ds, standardise = load_dataset(args, raw=True) if args.sparse_features else (load_dataset(args), False)
    if not args.quiet:
        print(args)
        print(f"dataset {ds.name}: N={ds.n_nodes} F={ds.x.shape[1]} edge rows={ds.src.size}")
    if args.sparse_features:
        from .features import SparseFeatures
        x = SparseFeatures.from_dense(ds.x, standardise=standardise).to(device)
        if not args.quiet:
            print(f"sparse features: {x.nnz} non-zero entries of {x.shape[0]} x {x.shape[1]}"
                  f"{', row-standardised' if standardise else ''}")
    else:
        x = torch.from_numpy(ds.x).to(device)
    tdt = torch.bfloat16 if args.table_dtype == "bf16" else torch.float32
    sdt = scan_table_dtype(args)
    result = []
    ranking = []
    global_ranking = []
    if (args.rank_eval or args.mine or args.global_rank_eval or args.predict_links is not None or
            args.predict_top is not None):                               # filter: every dataset edge, both directions
        s_all, d_all = torch.from_numpy(np.asarray(ds.src)).long(), torch.from_numpy(np.asarray(ds.dst)).long()
        known = (torch.cat([s_all, d_all]).to(device), torch.cat([d_all, s_all]).to(device))
    node_filter = load_node_groups(args.node_groups, ds.n_nodes, args.link_rule, device) if args.link_rule else None
    for run in range(args.run):
        if not args.quiet:
            print("run:", run)
        split = make_link_split(ds.src, ds.dst, ds.n_nodes, m=args.m, seed=args.seed + run)
        prepared = prepare_run(split, device, row_bytes=args.nfactor * args.nembed * (2 if args.table_dtype == "bf16" else 4),
                               resample_negatives=resample)
        torch.manual_seed(args.seed + run)
        model = Disentangle(x.shape[1], args.nhidden, args.nembed, nfactor=args.nfactor, beta=args.beta,
                            t=args.temperature, table_dtype=tdt).to(device)
        res = run_link_prediction(model, x, prepared, epochs=args.epochs, lr=args.lr,
                                  log=None if args.quiet else print,
                                  use_graph=_use_graph(args) and args.objective not in ("recon", "recon-logit")
                                  and not resample, objective=args.objective,
                                  resample_negatives=args.resample_negatives and args.objective != "bpr",
                                  resample_seed=args.resample_seed + run, hard_negatives=args.hard_negatives,
                                  pos_weight=args.pos_weight, recon_block_rows=args.recon_block_rows,
                                  recon_node_filter=node_filter if args.recon_link_rule else None)
        if not args.quiet:
            if resample:
                print("failed draws:", res.failed_draws)
            print("test auc:", res.test_auc)
        result.append(res.test_auc)
        if args.rank_eval:
            ranking.append(rank_eval(model, x, prepared.graph, split, known, node_filter, table_dtype=sdt))
            if not args.quiet:
                print("test ranking:", _fmt_ranking(ranking[-1]))
        if args.global_rank_eval:
            global_ranking.append(global_rank_eval(model, x, prepared.graph, split, known, node_filter, table_dtype=sdt))
            if not args.quiet:
                print("test global ranking:", _fmt_ranking(global_ranking[-1]))
    if args.mine and args.run > 0:                                  # the last run's model, its best weights
        mine_links(model, x, prepared.graph, known, args.mine, args.mine_out, node_filter=node_filter, table_dtype=sdt,
                   explained=args.explain)
    if args.predict_links is not None and args.run > 0:
        predict_links(model, x, prepared.graph, known, args.predict_links, args.links_out, node_filter=node_filter,
                      table_dtype=sdt, explained=args.explain)
    if args.predict_top is not None and args.run > 0:
        predict_top_links(model, x, prepared.graph, known, args.predict_top, args.links_out, node_filter=node_filter,
                          table_dtype=sdt, explained=args.explain)
    result = np.array(result)
    tail = []                                                       # the run means of the ranking metrics join the final line
    if args.rank_eval:
        tail.append(_fmt_ranking({key: float(np.mean([r[key] for r in ranking])) for key in ranking[0]}))
    if args.global_rank_eval:
        tail.append(_fmt_ranking({key: float(np.mean([r[key] for r in global_ranking])) for key in global_ranking[0]}))
    print("final", result.mean(), result.std(), *tail)
    if args.save == 1:                                              # :225-246
        save_results(args, result)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
