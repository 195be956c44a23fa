"""What the tests of the reconstruction loss under a node-group rule share (tests/test_recon_filter_cpu.py,
tests/test_gpu_recon_filter.py): the rules, the dense form of a rule and the references restricted by it.

The fp64 reference of a rule is the unfiltered one with every denied pair ignored: ``recon_ref.recon64(Z, H, t, pos,
ign | ~A)`` (logit space: ``recon_logits_ref.recon_logits64``) with A[u][v] = ``nf.allowed(u, v, unordered=True)``.  The bands
are therefore recon_ref's own, derived there; nothing here is tuned.
"""
import torch

import recon_ref

RULES = ("same3", "different3", "between", "candidates", "only63", "deny")
PLACED = ("tiles", "alternating")                  # ``different`` on placed groups (the GPU grid)


def make_rule(name, N, device="cpu"):
    """The rule ``name`` over N nodes as an ``ops.NodeFilter`` on ``device`` (CPU tensors in, deterministic in N):
      same3 / different3  three random groups;
      between             two random masks that overlap (and leave some nodes in neither);
      candidates          a random pool of about two thirds of the nodes;
      only63              64 groups, the only allowed pair of groups is (63, 63): bit 63 of allow word 63;
      deny                one group that may not link to itself: nothing is included;
      tiles               ``different`` on groups constant over whole 128-node tiles: whole tile pairs are denied;
      alternating         ``different`` on groups alternating node by node: every mask word is mixed;
      all                 one group, everything allowed: the rule that changes nothing."""
    from disenlink_amd.ops import NodeFilter
    gen = torch.Generator().manual_seed(1000 + N)
    if name in ("same3", "different3"):
        g = torch.randint(0, 3, (N,), generator=gen)
        g[0] = 2                                                   # n_groups = 3 whatever N
        return (NodeFilter.same if name == "same3" else NodeFilter.different)(g, device=device)
    if name == "between":
        a, b = torch.rand(N, generator=gen) < 0.6, torch.rand(N, generator=gen) < 0.6
        return NodeFilter.between(a, b, device=device)
    if name == "candidates":
        return NodeFilter.candidates(torch.rand(N, generator=gen) < 0.66, device=device)
    if name == "only63":
        g = torch.randint(0, 64, (N,), generator=gen)
        g[::3] = 63
        g[N - 1] = 63
        allow = torch.zeros(64, 64, dtype=torch.bool)
        allow[63, 63] = True
        return NodeFilter(g, allow, device=device)
    if name == "deny":
        return NodeFilter(torch.zeros(N, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.bool), device=device)
    if name == "tiles":
        return NodeFilter.different((torch.arange(N) // 128) % 2, device=device)      # N = 300: tile pairs (0,0) (1,1) (2,2) (0,2)
    if name == "alternating":
        return NodeFilter.different(torch.arange(N) % 2, device=device)
    if name == "all":
        return NodeFilter(torch.zeros(N, dtype=torch.int64), torch.ones(1, 1, dtype=torch.bool), device=device)
    raise KeyError(name)


def allowed_matrix(nf):
    """A [N,N] bool on the CPU: A[u][v] = nf.allowed(u, v, unordered=True)."""
    N = nf.n_nodes
    u, v = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    return nf.to("cpu").allowed(u.reshape(-1), v.reshape(-1), unordered=True).reshape(N, N)


def pairs_of(rowptr, col):
    """The (row, column) entries of a CSR as a set."""
    if rowptr is None:
        return set()
    rp, c = rowptr.tolist(), col.tolist()
    return {(u, c[i]) for u in range(len(rp) - 1) for i in range(rp[u], rp[u + 1])}


# The rule of the module-level checks.  On recon_ref.MODULE_CASES a plain fp32 CPU evaluation of the dense formulation stays
# within a quarter of the GPU test's tolerance of the fp64 one under it (tests/test_recon_filter_cpu.py holds it to that):
#   k8_d64   226 + 1174 of 407 + 2015 pairs   loss 1.2e-07  gradients 3.6e-07
#   tiny_k1    6 + 6    of   8 + 13           loss 3.1e-08  gradients 1.5e-07
# ("alternating" was looked at first: its fp32 loss sum on k8_d64 stands 4.4e-06 from fp64, too close to the 5e-06 allowed.)
MODULE_RULE = "between"


def module_reference(g, A, dtype=torch.float64):
    """``recon_ref.module_reference`` with its included pairs restricted by ``A`` (bool [N,N], symmetric): CPU autograd of the
    oracle's dense forward under the masked, weighted BCE over the upper triangle, positives = the edges of the case's
    adjacency, ignored = pair_sets(N, seed=N)[1] and every pair A denies, pos_weight = n_neg / n_pos of what remains
    -> (loss, {parameter: gradient}, ign, (n_pos, n_neg), entries of P among them that are exactly 0 or 1)."""
    from oracle import dense_ref
    m = g["meta"]
    N = m["N"]
    adj = torch.from_numpy(g["adj"])
    pos = (adj != 0) | (adj.t() != 0)
    _p, ign = recon_ref.pair_sets(N, seed=N)
    inc = torch.triu(~ign & A, diagonal=1)
    y = (pos & inc).to(dtype)
    n_pos = int(y.sum())
    n_neg = int(inc.sum()) - n_pos
    weight = torch.where(y > 0, torch.tensor(n_neg / n_pos / (n_pos + n_neg), dtype=dtype),
                         torch.tensor(1.0 / (n_pos + n_neg), dtype=dtype)) * inc
    sd = {k[4:]: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in g.items() if k.startswith("sd__")}
    _e, P = dense_ref.forward(torch.from_numpy(g["x"]).to(dtype), adj.to(dtype), sd, m["beta"], m["t"])
    loss = torch.nn.functional.binary_cross_entropy(P, y, weight=weight, reduction="sum")
    loss.backward()
    saturated = int(((P == 0) | (P == 1))[inc].sum())
    return float(loss.detach()), {k: v.grad.double() for k, v in sd.items()}, ign, (n_pos, n_neg), saturated
