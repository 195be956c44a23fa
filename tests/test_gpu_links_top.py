"""The budgeted link graph (ops.score_top_links, Disentangle.top_predicted_links, --predict-top): exact against the
enumerated pairs (ops.score_pair_logits + links_top_ref.select_top_links) for budgets below and above the mining's cap,
the list ops.score_mine gives, ties across the cut, exclusion and node-group rules, special values, bf16 tables,
reproducibility, the short fill, the refusals, the reference model's own link_pred (tests/golden) and the CLI."""
import contextlib
import io

import numpy as np
import pytest
import torch

import links_ref
import links_top_ref
from conftest import golden_case_names, load_golden
from links_ref import upper_pairs
from links_top_ref import select_top_links
from test_gpu_links import DEV, INF, NINF, POISON_BITS, assert_layout, bits, enumerate_logits, same, tables

pytestmark = pytest.mark.gpu


def prob_bits_of(full, N):
    """[N,N] int32: the bits of prob that a links call lists for every (row, col) it holds, 0 elsewhere"""
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), full[0][1:] - full[0][:-1])
    P = torch.zeros(N, N, dtype=torch.int32, device=DEV)
    P[rows, full[1].long()] = bits(full[3])
    return P


def assert_equals_reference(out, S, N, m, full, excluded=None, floor=NINF):
    """rowptr, col and the bits of logit are links_top_ref.select_top_links', prob has the bits ops.score_links lists for the
    pair (``full``: its result without a floor), and there are 2 min(m, eligible) entries"""
    assert_layout(out, N)
    rowptr, col, logit, prob = out
    rp, rc, rl = select_top_links(S, m, excluded, floor)
    assert torch.equal(rowptr, rp) and torch.equal(col.long(), rc) and torch.equal(bits(logit), bits(rl))
    eligible = len(upper_pairs(*links_ref.select_links(S, excluded, floor))[0])
    assert int(rowptr[-1]) == 2 * min(m, eligible)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), rowptr[1:] - rowptr[:-1])
    assert torch.equal(bits(prob), prob_bits_of(full, N)[rows, col.long()])


@pytest.mark.parametrize("N,KD,t", links_top_ref.GPU_CASES)
def test_exact_against_the_enumerated_pairs(N, KD, t):
    from disenlink_amd import ops
    K, d = KD
    Z, H = tables(N, K, d, seed=links_ref.case_seed(N, K, d, t))
    S = enumerate_logits(Z, H, t)
    full = ops.score_links(Z, H, t, NINF)
    for m in links_top_ref.gpu_m_values(N):
        assert_equals_reference(ops.score_top_links(Z, H, t, m), S, N, m, full)


@pytest.mark.parametrize("KD", links_top_ref.BIG_KD)
def test_budgets_beyond_the_cap_of_the_mining(KD):
    from disenlink_amd import ops
    N, (K, d), t = links_top_ref.BIG_N, KD, 1.0
    Z, H = tables(N, K, d, seed=links_ref.case_seed(N, K, d, 1))
    S = enumerate_logits(Z, H, t)
    full = ops.score_links(Z, H, t, NINF)
    for m in links_top_ref.BIG_M:
        assert m > ops.MINE_MAX_M
        out = ops.score_top_links(Z, H, t, m)
        assert len(out[1]) == 2 * m
        assert_equals_reference(out, S, N, m, full)


@pytest.mark.parametrize("N", [129, 300])
def test_the_upper_pairs_are_the_list_of_score_mine(N):
    from disenlink_amd import ops
    K, d, t, m = 3, 40, 2.0, 1000
    Z, H = tables(N, K, d, seed=21 + N)
    ex = (torch.tensor([0, 3, N - 1, 128], device=DEV), torch.tensor([2, 1, 0, 5], device=DEV))
    for exclude in (None, ex):
        for floor in (NINF, 0.05):
            u, v, logit, prob = upper_pairs(*ops.score_top_links(Z, H, t, m, exclude=exclude, min_logit=floor))
            src, dst, lg, pr = ops.score_mine(Z, H, t, m, exclude=exclude, min_logit=floor)
            assert len(src) == len(u) == m
            order = torch.argsort(src.long() * N + dst.long())
            assert torch.equal(u, src.long()[order]) and torch.equal(v, dst.long()[order])
            assert torch.equal(bits(logit), bits(lg[order])) and torch.equal(bits(prob), bits(pr[order]))


def test_ties_across_the_cut_go_to_the_smaller_pair_index():
    from disenlink_amd import ops
    # repeated node rows: whole classes of pairs tie exactly
    N, K, d = 260, 2, 32
    Z, H = tables(N, K, d, seed=41)
    base = torch.arange(N, device=DEV) % 13                           # 13 distinct rows, each 20 times
    Z, H = Z[base].contiguous(), H[base].contiguous()
    S = enumerate_logits(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    vals, counts = torch.unique(S[iu], return_counts=True)
    assert len(vals) <= 13 * 13 and int(counts.min()) >= 100          # a class per pair of distinct rows, in either order
    full = ops.score_links(Z, H, 1.0, NINF)
    order = torch.argsort(vals, descending=True)
    above = 0
    for i in order[:4].tolist():                                      # a cut inside each of the four best classes
        c = int(counts[i])
        for m in (above + 1, above + c // 2, above + c - 1):
            out = ops.score_top_links(Z, H, 1.0, m)
            assert_equals_reference(out, S, N, m, full)
            u, v, logit = upper_pairs(out[0], out[1], out[2])
            tied = logit == vals[i]
            assert int(tied.sum()) == m - above and int((logit > vals[i]).sum()) == above
            # the chosen of the class are its first by u * N + v
            cu, cv = torch.nonzero(iu & (S == vals[i]), as_tuple=True)
            assert torch.equal(u[tied], cu[:m - above]) and torch.equal(v[tied], cv[:m - above])
        above += c
    # an all-equal table: every logit is equal, the chosen pairs are the first m in row-major order
    N = 140
    Z, H = torch.full((N, 1, 8), 0.25, device=DEV), torch.full((N, 1, 8), 0.5, device=DEV)
    S = enumerate_logits(Z, H, 1.0)
    assert len(torch.unique(S[torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)])) == 1
    full = ops.score_links(Z, H, 1.0, NINF)
    au, av = torch.triu_indices(N, N, 1, device=DEV)
    for m in (1, 138, 139, 140, 5000, N * (N - 1) // 2 - 1):
        out = ops.score_top_links(Z, H, 1.0, m)
        assert_equals_reference(out, S, N, m, full)
        u, v = upper_pairs(out[0], out[1])
        assert torch.equal(u, au[:m]) and torch.equal(v, av[:m])


def test_exclusion_forms_agree_and_either_orientation_counts():
    from disenlink_amd import ops
    from disenlink_amd.graph import Graph
    N, K, d, m = 150, 3, 64, 3000
    Z, H = tables(N, K, d, seed=3)
    rng = np.random.default_rng(3)
    s, t_ = torch.from_numpy(rng.integers(0, N, 2500)).to(DEV), torch.from_numpy(rng.integers(0, N, 2500)).to(DEV)
    mask = torch.zeros(N, N, device=DEV)
    mask[s, t_] = 1                                                   # one orientation only
    G = Graph.from_edge_rows(s, t_, N)
    S = enumerate_logits(Z, H, 1.0)
    full = ops.score_links(Z, H, 1.0, NINF)
    prepared = [ops.pair_exclusion((s, t_), N, DEV), ops.pair_exclusion((t_, s), N, DEV), ops.pair_exclusion(mask, N, DEV)]
    for floor in (NINF, 0.0):
        outs = [ops.score_top_links(Z, H, 1.0, m, exclude=e, min_logit=floor) for e in [G, mask, (s, t_), (t_, s)] + prepared]
        assert all(same(outs[0], o) for o in outs[1:])
        assert_equals_reference(outs[0], S, N, m, full, mask.bool(), floor)
    none = ops.pair_exclusion(None, N, DEV)                           # a prepared empty set
    assert same(ops.score_top_links(Z, H, 1.0, m, exclude=none), ops.score_top_links(Z, H, 1.0, m))
    with pytest.raises(ValueError, match="exclusion set of 150 nodes, expected 10"):
        ops.score_top_links(Z[:10], H[:10], 1.0, m, exclude=prepared[0])
    # the best pair of all, excluded as (v, u) only: the budget moves on to the next
    free = ops.score_top_links(Z, H, 1.0, 1)
    u, v = (int(x[0]) for x in upper_pairs(free[0], free[1]))
    only = ops.score_top_links(Z, H, 1.0, 1, exclude=(torch.tensor([v]), torch.tensor([u])))
    one = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    one[u, v] = True
    assert_equals_reference(only, S, N, 1, full, one)
    assert tuple(int(x[0]) for x in upper_pairs(only[0], only[1])) != (u, v)


@pytest.mark.parametrize("N,K,d,t", [(N, K, d, t) for N in (1, 130, 300) for K, d, t in ((1, 8, 1.0), (3, 64, 2.0))])
def test_node_filter_equals_the_rule_as_exclusion(N, K, d, t):
    """every NodeFilter rule of test_gpu_node_filter.py: the bits of the unfiltered call with the disallowed pairs excluded"""
    from disenlink_amd import ops
    from test_gpu_node_filter import unordered_cases
    Z, H = tables(N, K, d, seed=N + 7 * K + d + 2)
    for name, f, allowed, ex, n_cand in unordered_cases(N, seed=N + 2):
        for m in (5, max(1, n_cand // 2), n_cand + 10):
            got = ops.score_top_links(Z, H, t, m, exclude=ex, node_filter=f)
            want = ops.score_top_links(Z, H, t, m, exclude=ex | ~allowed)
            assert same(got, want), (name, m)
            u, v = upper_pairs(got[0], got[1])
            assert bool(allowed[u, v].all()) and len(u) == min(m, n_cand), name
            if m > n_cand:
                assert same(got, ops.score_links(Z, H, t, NINF, exclude=ex, node_filter=f)), name


def test_a_floor_or_a_budget_above_the_candidates_gives_score_links():
    from disenlink_amd import ops
    N, K, d = 300, 2, 32
    Z, H = tables(N, K, d, seed=17)
    at_floor = ops.score_links(Z, H, 1.0, 0.1)
    n = len(at_floor[1]) // 2
    assert 100 < n < N * (N - 1) // 2 - 100
    for m in (n, n + 1, 3 * n, 1 << 40):                              # min_logit AND the budget: fewer than m pairs reach the floor
        assert same(ops.score_top_links(Z, H, 1.0, m, min_logit=0.1), at_floor)
    short = ops.score_top_links(Z, H, 1.0, n - 7, min_logit=0.1)
    assert len(short[1]) == 2 * (n - 7) and float(short[2].min()) >= 0.1
    everything = ops.score_links(Z, H, 1.0, NINF)
    for m in (N * (N - 1) // 2, N * (N - 1) // 2 + 1, (1 << 63) - 1, 1 << 70):
        assert same(ops.score_top_links(Z, H, 1.0, m), everything)


def test_infinities_first_nan_never_and_zeros_of_either_sign():
    from disenlink_amd import ops
    N, d = 90, 32
    Z, H = tables(N, 1, d, seed=7)
    Z[:45] = 4.0                                                      # z.z = 512: exp overflows
    H[:20] = 0.25                                                     # h.h > 0: +inf
    H[20:30] = 0.25
    H[20:30, :, ::2] = -0.5                                           # against rows 0..19: h.h < 0: -inf
    H[30:45] = 0.0                                                    # h.h = 0 against inf: NaN
    S = enumerate_logits(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_pinf, n_ninf, n_nan = int((iu & (S == INF)).sum()), int((iu & (S == NINF)).sum()), int((iu & torch.isnan(S)).sum())
    assert n_pinf >= 190 and n_ninf >= 200 and n_nan >= 15 * 30
    total = N * (N - 1) // 2
    full = ops.score_links(Z, H, 1.0, NINF)
    for m in (1, n_pinf - 3, n_pinf, n_pinf + 5, total - n_nan - n_ninf + 4, total - n_nan, total):
        out = ops.score_top_links(Z, H, 1.0, m)
        assert_equals_reference(out, S, N, m, full)
        assert len(out[1]) == 2 * min(m, total - n_nan) and not torch.isnan(out[2]).any() and not torch.isnan(out[3]).any()
        assert int((out[2] == INF).sum()) == 2 * min(m, n_pinf)       # +inf is taken first
        assert int((out[2] == NINF).sum()) == 2 * max(0, min(m, total - n_nan) - (total - n_nan - n_ninf))      # -inf last
    # zeros of either sign: one class of ties, reported as +0
    N, K, d = 200, 2, 32
    Z, H = tables(N, K, d, seed=31)
    zero = torch.from_numpy(np.random.default_rng(31).choice(N, 120, replace=False)).to(DEV)
    H[zero] = 0.0
    H[zero[:40], :, ::2] = -0.0
    S = enumerate_logits(Z, H, 1.0)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    n_pos, n_zero = int((iu & (S > 0)).sum()), int((iu & (S == 0)).sum())
    assert n_zero > 5000
    full = ops.score_links(Z, H, 1.0, NINF)
    m = n_pos + n_zero // 3                                           # the cut falls inside the run of zeros
    out = ops.score_top_links(Z, H, 1.0, m)
    assert_equals_reference(out, S, N, m, full)
    assert int((out[2] == 0).sum()) == 2 * (n_zero // 3) and not torch.signbit(out[2]).any()


@pytest.mark.parametrize("N,K,d", [(1, 1, 8), (2, 3, 40), (129, 2, 96), (300, 8, 64)])
def test_bf16_tables_give_the_bits_of_the_fp32_call_on_the_widened_tables(N, K, d):
    from disenlink_amd import ops
    Z, H = tables(N, K, d, seed=N + K + d)
    Zb, Hb = Z.bfloat16(), H.bfloat16()
    for m in (1, max(1, N * (N - 1) // 4), N * N):
        want = ops.score_top_links(Zb.float(), Hb.float(), 1.0, m)
        assert same(ops.score_top_links(Zb, Hb, 1.0, m, table_dtype=torch.bfloat16), want)
        assert same(ops.score_top_links(Z, H, 1.0, m, table_dtype=torch.bfloat16), want)        # fp32 tensors are rounded
    f = ops.NodeFilter.different(torch.arange(N) % 3, device=DEV)
    m = max(1, N * (N - 1) // 6)
    assert same(ops.score_top_links(Zb, Hb, 1.0, m, node_filter=f, table_dtype=torch.bfloat16),
                ops.score_top_links(Zb.float(), Hb.float(), 1.0, m, node_filter=f))


def test_n_of_one_and_two():
    from disenlink_amd import ops
    Z, H = tables(1, 2, 8, seed=1)
    for m in (1, 5):
        out = ops.score_top_links(Z, H, 1.0, m)
        assert_layout(out, 1)
        assert out[0].tolist() == [0, 0] and len(out[1]) == 0
    Z, H = tables(2, 2, 8, seed=2)
    x = ops.score_pair_logits(Z, H, 1.0, torch.tensor([0]), torch.tensor([1]))
    for m in (1, 2):
        out = ops.score_top_links(Z, H, 1.0, m)
        assert out[0].tolist() == [0, 1, 2] and out[1].tolist() == [1, 0] and torch.equal(bits(out[2]), bits(torch.cat([x, x])))
    assert ops.score_top_links(Z, H, 1.0, 1, min_logit=float(x) + 1.0)[0].tolist() == [0, 0, 0]
    assert ops.score_top_links(Z, H, 1.0, 1, exclude=(torch.tensor([1]), torch.tensor([0])))[0].tolist() == [0, 0, 0]


def test_bitwise_reproducible_under_any_geometry(lib_env):
    from disenlink_amd import _lib, ops
    N, K, d, m = 700, 3, 64, 90000                                    # 6 tiles, 21 tile pairs; a budget above the mining's cap
    Z, H = tables(N, K, d, seed=13)
    H[100:400] = 0.0                                                  # 164,850 zero logits: the cut falls inside their tie class
    excl = (torch.arange(N, device=DEV), (torch.arange(N, device=DEV) + 1) % N)
    f = ops.NodeFilter.different(torch.arange(N) % 5, device=DEV)
    ref = ops.score_top_links(Z, H, 1.0, m, exclude=excl)
    ref_f = ops.score_top_links(Z, H, 1.0, m, exclude=excl, node_filter=f)
    assert_layout(ref, N)
    assert len(ref[1]) == 2 * m == len(ref_f[1]) and int((ref[2] == 0).sum()) > 1000 and int((ref[2] > 0).sum()) > 1000
    assert int(ref[1].min()) >= 0 and int(ref[1].max()) < N
    assert not (bits(ref[2]) == POISON_BITS).any() and not (bits(ref[3]) == POISON_BITS).any()      # every slot was written
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), ref[0][1:] - ref[0][:-1])
    key = rows * N + ref[1].long()
    assert (key[1:] > key[:-1]).all() and (rows != ref[1]).all()
    assert same(ref, ops.score_top_links(Z, H, 1.0, m, exclude=excl))
    for tiles in (1, 3, 21):                                          # DL_MINE_TILES: tile pairs per workgroup (21 = all of them)
        lib_env("DL_MINE_TILES", tiles)
        assert _lib.score_links_top_form(N, K, d)["pairs_per_wg"] == tiles
        assert same(ref, ops.score_top_links(Z, H, 1.0, m, exclude=excl))
        assert same(ref_f, ops.score_top_links(Z, H, 1.0, m, exclude=excl, node_filter=f))
    lib_env("DL_MINE_TILES")
    lib_env("DL_POISON", 1)
    assert same(ref, ops.score_top_links(Z, H, 1.0, m, exclude=excl))
    # the same set as score_links at the floor of the m-th logit, less the ties the budget cuts off
    floor = float(ref[2].min())
    at_floor = ops.score_links(Z, H, 1.0, floor, exclude=excl)
    assert floor == 0.0 and len(at_floor[1]) > len(ref[1])
    above = ops.score_links(Z, H, 1.0, float(np.nextafter(np.float32(floor), np.float32(INF))), exclude=excl)
    assert 0 < len(above[1]) < len(ref[1])


def test_scans_that_ran_are_counted_and_at_most_six():
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d = 300, 2, 32
    Z, H = tables(N, K, d, seed=17)
    form = _lib.score_links_top_form(N, K, d)
    ws = torch.zeros(int(lib.dl_score_links_top_workspace_bytes_dtype(N, K, d, 0)), dtype=torch.uint8, device=DEV)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    off = (-ws.data_ptr()) % 256 + form["scans_offset"]
    for m, most in ((N * N, 1), (1000, 6), (1, 6)):                   # every candidate: the first pick ends the search
        head = (Z.data_ptr(), H.data_ptr(), N, K, d, 0, 1.0, None, None, NINF, m, None, ws.data_ptr(), ws.numel(), rowptr.data_ptr())
        assert lib.dl_score_links_top_count_dtype(*head, ops._stream()) == 0
        ran = int(ws[off:off + 4].view(torch.int32).item())
        assert 1 <= ran <= most and ran + 2 <= form["scans"]
        assert int(rowptr[-1]) == 2 * min(m, N * (N - 1) // 2)


def test_a_short_fill_writes_nothing_out_of_bounds():
    """dl_score_links_top_fill_dtype with an nnz below the count's: slots >= nnz are skipped, the slots below it are the same bits"""
    from disenlink_amd import _lib, ops
    lib = _lib.load()
    N, K, d, m = 300, 2, 32, 9000
    Z, H = tables(N, K, d, seed=17)
    full = ops.score_top_links(Z, H, 1.0, m)
    nnz = len(full[1])
    assert nnz == 2 * m
    ws = torch.full((int(lib.dl_score_links_top_workspace_bytes_dtype(N, K, d, 0)),), 0x7F, dtype=torch.uint8, device=DEV)
    rowptr = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    head = (Z.data_ptr(), H.data_ptr(), N, K, d, 0, 1.0, None, None, NINF, m, None, ws.data_ptr(), ws.numel(), rowptr.data_ptr())
    assert lib.dl_score_links_top_count_dtype(*head, ops._stream()) == 0
    assert torch.equal(rowptr, full[0])
    short = nnz // 2
    col = torch.full((nnz,), -5, dtype=torch.int32, device=DEV)
    logit = torch.full((nnz,), -5.0, device=DEV)
    assert lib.dl_score_links_top_fill_dtype(*head, short, col.data_ptr(), logit.data_ptr(), None, ops._stream()) == 0      # prob not wanted
    assert torch.equal(col[:short], full[1][:short]) and torch.equal(bits(logit[:short]), bits(full[2][:short]))
    assert (col[short:] == -5).all() and (logit[short:] == -5.0).all()
    assert lib.dl_score_links_top_fill_dtype(*head, 0, None, None, None, ops._stream()) == 0


def test_argument_errors():
    from disenlink_amd import ops, _lib
    lib = _lib.load()
    Z, H = tables(10, 2, 32)
    for m in (0, -1):
        with pytest.raises(_lib.DisenlinkHipError, match=r"code -1\).*below 1"):
            ops.score_top_links(Z, H, 1.0, m)
    with pytest.raises(ValueError, match="46340"):
        big = torch.zeros(46341, 1, 1, device=DEV)
        ops.score_top_links(big, big, 1.0, 5)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    rowptr = torch.zeros(11, dtype=torch.int64, device=DEV)
    big = torch.zeros(46341, 1, 1, device=DEV)
    assert lib.dl_score_links_top_count_dtype(big.data_ptr(), big.data_ptr(), 46341, 1, 1, 0, 1.0, None, None, 0.0, 5, None,
                                              ws.data_ptr(), ws.numel(), rowptr.data_ptr(), ops._stream()) == -1
    assert b"outside 1..46340" in lib.dl_last_error()
    need = int(lib.dl_score_links_top_workspace_bytes_dtype(10, 2, 32, 0))
    assert lib.dl_score_links_top_count_dtype(Z.data_ptr(), H.data_ptr(), 10, 2, 32, 0, 1.0, None, None, 0.0, 5, None,
                                              ws.data_ptr(), need - 1, rowptr.data_ptr(), ops._stream()) == -3
    assert b"workspace too small" in lib.dl_last_error()
    f = ops.NodeFilter.different(torch.arange(10) % 2)                # on the CPU
    with pytest.raises(ValueError, match="use NodeFilter.to"):
        ops.score_top_links(Z, H, 1.0, 5, node_filter=f)
    with pytest.raises(_lib.DisenlinkHipError):
        Zw, Hw = tables(10, 1, 130)
        ops.score_top_links(Zw, Hw, 1.0, 5)
    with pytest.raises(_lib.DisenlinkHipError, match="temperature is 0"):
        ops.score_top_links(Z, H, 0.0, 5)


@pytest.mark.parametrize("name", golden_case_names())
def test_top_predicted_links_against_the_reference_link_pred(name):
    """With p* the m-th largest reference probability among the candidates: every chosen pair has a reference probability
    >= p* less test_gpu_parity.py's tolerance for link_pred (rtol = atol = 1e-5), every other candidate one <= p* plus it;
    the saturated fixtures check the count and the layout"""
    from disenlink_amd.model import Disentangle, PredictedLinks
    g = load_golden(name)
    meta = g["meta"]
    model = Disentangle(meta["F"], meta["nhid"], meta["d"], nfactor=meta["K"], beta=meta["beta"], t=meta["t"])
    model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")})
    model = model.to(DEV)
    x, adj = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["adj"]).to(DEV)
    N, m = meta["N"], links_top_ref.GOLDEN_M[name]
    lp = g["link_pred"]
    ref = torch.from_numpy(lp).double().to(DEV)
    iu = torch.triu(torch.ones(N, N, dtype=torch.bool, device=DEV), 1)
    edges = adj.bool() | adj.bool().T
    none = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    for exclude, cand in ((none, iu), (None, iu & ~edges)):
        links = model.top_predicted_links(x, adj, m, exclude=exclude)
        assert isinstance(links, PredictedLinks) and links.n_nodes == N
        assert_layout(links, N)
        u, v, logit, prob = links.pairs()
        got = torch.zeros(N, N, dtype=torch.bool, device=DEV)
        got[u, v] = True
        assert len(u) == m == int(got.sum()) and not (got & ~cand).any()
        assert torch.equal(links.degree, (got | got.T).sum(1))
        np.testing.assert_allclose(prob.cpu().numpy(), lp[u.cpu().numpy(), v.cpu().numpy()], rtol=1e-5, atol=1e-5)
        if name in links_top_ref.GOLDEN_SATURATED:
            continue
        p, doubt = links_top_ref.golden_cut(lp, cand.cpu().numpy(), m)
        tol = 1e-5 + 1e-5 * p
        print(f"{name}: p* = {p:.9g}, chosen min {float(ref[got].min()):.9g}, others max {float(ref[cand & ~got].max()):.9g}, "
              f"in doubt {int(doubt.sum())} of {int(cand.sum())}")
        assert int(doubt.sum()) <= links_top_ref.doubt_cap(int(cand.sum()))
        assert bool((ref[got] >= p - tol).all()) and bool((ref[cand & ~got] <= p + tol).all())
    given = model.top_predicted_links(x, adj, m, exclude=torch.nonzero(edges, as_tuple=True))
    assert same(links, given)                                         # exclude=None: the edges of adj
    with_floor = model.top_predicted_links(x, adj, 10 * N * N, min_prob=0.5)
    assert same(with_floor, model.predicted_links(x, adj, 0.5))       # the budget does not bind: the thresholded graph


def test_cli_predict_top_prints_and_writes_what_the_module_gives(tmp_path):
    from disenlink_amd import main as cli
    groups = tmp_path / "groups.txt"
    ds = cli.load_dataset(cli.build_parser().parse_args(["--dataset", "squirrel", "--synthetic"]))
    groups.write_text("\n".join(str(i % 3) for i in range(ds.n_nodes)) + "\n")
    out = tmp_path / "links.txt"
    seen = {}
    real, real_explain = cli.predict_top_links, cli.explain

    def spy(*args, **kwargs):
        seen["links"] = real(*args, **kwargs)
        return seen["links"]

    def spy_explain(*args, **kwargs):
        seen["factor"] = real_explain(*args, **kwargs)
        return seen["factor"]
    cli.predict_top_links, cli.explain = spy, spy_explain
    buf = io.StringIO()
    m = 70000                                                         # above the cap of --mine
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(["--dataset", "squirrel", "--synthetic", "--epochs", "1", "--run", "1", "--quiet", "--predict-top", str(m),
                      "--links-out", str(out), "--node-groups", str(groups), "--link-rule", "different", "--explain"])
    finally:
        cli.predict_top_links, cli.explain = real, real_explain
    links = seen["links"]
    src, dst, _, prob = (t.cpu().numpy() for t in links.pairs())
    lines = buf.getvalue().splitlines()
    line = [ln for ln in lines if ln.startswith("predicted ") and " links under a budget of " in ln]
    assert len(line) == 1 and len([ln for ln in lines if ln.startswith("predicted links by dominant factor:")]) == 1
    words = line[0].split()
    n = ds.n_nodes
    deg = links.degree.cpu().numpy()
    assert int(words[1]) == len(src) == m and words[2] == "links" and words[words.index("of") + 1] == f"{m}:"
    assert float(words[words.index("density") + 1]) == pytest.approx(len(src) / (n * (n - 1) / 2), rel=1e-5)
    assert float(words[words.index("mean") + 2]) == pytest.approx(deg.mean(), rel=1e-5) and int(words[-1]) == deg.max()
    rows = [ln.split() for ln in out.read_text().splitlines()]
    assert len(rows) == len(src) and all(len(r) == 4 for r in rows)   # --explain: `src dst prob factor`
    assert [int(r[0]) for r in rows] == src.tolist() and [int(r[1]) for r in rows] == dst.tolist()
    np.testing.assert_allclose([float(r[2]) for r in rows], prob, rtol=1e-8)
    assert [int(r[3]) for r in rows] == seen["factor"][0].tolist()
    assert (src < dst).all() and (src % 3 != dst % 3).all()
    known = set(zip(np.asarray(ds.src).tolist(), np.asarray(ds.dst).tolist()))
    assert not any((a, b) in known or (b, a) in known for a, b in zip(src.tolist(), dst.tolist()))
