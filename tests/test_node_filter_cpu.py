"""ops.NodeFilter (the node-group rule of the candidate scans) on the host: its constructors, ``allowed``, symmetry, and
every refusal of a bad filter through the C ABI, through ``ops`` and through the CLI — all of them ahead of any launch, so
none of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_constructors_against_hand_written_rules():
    from disenlink_amd.ops import NodeFilter
    g = torch.tensor([0, 2, 1, 2, 0])
    f = NodeFilter.same(g)
    assert f.n_nodes == 5 and f.n_groups == 3 and f.symmetric and f.groups.dtype == torch.uint8
    assert f.allow.tolist() == [[True, False, False], [False, True, False], [False, False, True]]
    assert f._words.tolist() == [1, 2, 4]
    f = NodeFilter.different(g)
    assert f.symmetric and f.allow.tolist() == [[False, True, True], [True, False, True], [True, True, False]]
    assert f._words.tolist() == [6, 5, 3] and f._pair_words.tolist() == [6, 5, 3]
    a = torch.tensor([1, 1, 0, 0, 1], dtype=torch.bool)
    b = torch.tensor([0, 1, 1, 0, 0], dtype=torch.bool)
    f = NodeFilter.between(a, b)                                      # groups: 1 = a only, 2 = b only, 3 = both, 0 = neither
    assert f.groups.tolist() == [1, 3, 2, 0, 1] and f.n_groups == 4 and f.symmetric
    assert f.allow.tolist() == [[False] * 4, [False, False, True, True], [False, True, False, True], [False, True, True, True]]
    f = NodeFilter.between(a, b, both_ways=False)
    assert not f.symmetric and f.pair_allow is None
    assert f.allow.tolist() == [[False] * 4, [False, False, True, True], [False] * 4, [False, False, True, True]]
    f = NodeFilter.candidates(torch.tensor([0, 1, 1, 0, 0]))
    assert f.groups.tolist() == [0, 1, 1, 0, 0] and not f.symmetric
    assert f.allow.tolist() == [[False, True], [False, True]]          # ordered: any query, pool members only
    assert f.pair_allow.tolist() == [[False, False], [False, True]]    # unordered: both endpoints in the pool
    assert f._words.tolist() == [2, 2] and f._pair_words.tolist() == [0, 2]
    one = NodeFilter(torch.zeros(4, dtype=torch.int64), torch.ones(1, 1))
    assert one.n_groups == 1 and one.symmetric and one._words.tolist() == [1]


def test_bit_63_and_packing():
    from disenlink_amd.ops import NodeFilter
    allow = torch.zeros(64, 64, dtype=torch.bool)
    allow[31, 63] = allow[63, 31] = allow[32, 32] = allow[63, 63] = True
    f = NodeFilter(torch.tensor([31, 32, 63, 0]), allow)
    w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in f._words.tolist()]
    assert w[31] == 1 << 63 and w[32] == 1 << 32 and w[63] == (1 << 63) | (1 << 31) and w[0] == 0
    assert f.allowed(torch.tensor([0, 0, 1, 2, 3]), torch.tensor([2, 1, 1, 2, 3])).tolist() == [True, False, True, True, False]


def test_allowed_against_a_double_loop():
    from disenlink_amd.ops import NodeFilter
    N = 12
    gen = torch.Generator().manual_seed(5)
    groups = torch.randint(0, 5, (N,), generator=gen)
    allow = torch.rand(5, 5, generator=gen) < 0.5
    f = NodeFilter(groups, allow)
    u, v = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    got = f.allowed(u.reshape(-1), v.reshape(-1)).reshape(N, N)
    for a in range(N):
        for b in range(N):
            assert bool(got[a, b]) == bool(allow[int(groups[a]), int(groups[b])])
    sym = NodeFilter(groups, allow | allow.T)
    got = sym.allowed(u.reshape(-1), v.reshape(-1), unordered=True).reshape(N, N)
    assert torch.equal(got, got.T)
    n_pairs = sum(bool(got[a, b]) for a in range(N) for b in range(a + 1, N))
    assert int(sym._n_pairs_allowed()) == n_pairs
    pool = NodeFilter.candidates(groups < 2)
    got = pool.allowed(u.reshape(-1), v.reshape(-1), unordered=True).reshape(N, N)
    for a in range(N):
        for b in range(N):
            assert bool(got[a, b]) == (int(groups[a]) < 2 and int(groups[b]) < 2)
    assert int(pool._n_pairs_allowed()) == (lambda c: c * (c - 1) // 2)(int((groups < 2).sum()))


def test_symmetry_detection_and_constructor_errors():
    from disenlink_amd.ops import NodeFilter
    g = torch.tensor([0, 1, 1])
    assert NodeFilter(g, torch.tensor([[1, 1], [1, 0]])).symmetric
    asym = NodeFilter(g, torch.tensor([[0, 1], [0, 0]]))
    assert not asym.symmetric and asym.pair_allow is None
    with pytest.raises(ValueError, match="symmetric"):
        asym.allowed(torch.tensor([0]), torch.tensor([1]), unordered=True)
    moved = asym.to("cpu")
    assert moved.n_nodes == 3 and not moved.symmetric and torch.equal(moved.groups, asym.groups)
    with pytest.raises(ValueError, match="groups outside"):
        NodeFilter(torch.tensor([0, 2]), torch.ones(2, 2))
    with pytest.raises(ValueError, match="groups outside"):
        NodeFilter(torch.tensor([0, -1]), torch.ones(2, 2))
    for bad in (torch.ones(2, 3), torch.ones(2), torch.ones(65, 65), torch.ones(0, 0)):
        with pytest.raises(ValueError, match="allow must be"):
            NodeFilter(torch.tensor([0, 0]), bad)
    with pytest.raises(ValueError, match="1-D integer"):
        NodeFilter(torch.tensor([0.0, 1.0]), torch.ones(2, 2))
    with pytest.raises(ValueError, match="1-D integer"):
        NodeFilter(torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, 2))
    with pytest.raises(ValueError, match="0..63"):
        NodeFilter.different(torch.tensor([0, 64]))
    with pytest.raises(ValueError, match="one length"):
        NodeFilter.between(torch.ones(3), torch.ones(4))


def test_ops_refuse_a_bad_filter_before_anything_else():
    """the tables are on the CPU: a call that got as far as the kernels' own checks would fail with DisenlinkHipError"""
    from disenlink_amd import ops
    Z = torch.zeros(6, 2, 8)
    good = ops.NodeFilter.different(torch.tensor([0, 1, 0, 1, 0, 1]))
    asym = ops.NodeFilter(torch.tensor([0, 1, 0, 1, 0, 1]), torch.tensor([[0, 1], [0, 0]]))
    short = ops.NodeFilter.different(torch.tensor([0, 1, 0]))
    q = torch.tensor([0, 1])
    calls = {
        "score_topk": lambda f: ops.score_topk(Z, Z, 1.0, q, 2, node_filter=f),
        "score_ranks": lambda f: ops.score_ranks(Z, Z, 1.0, q, q.flip(0), node_filter=f),
        "score_mine": lambda f: ops.score_mine(Z, Z, 1.0, 3, node_filter=f),
        "score_pair_ranks": lambda f: ops.score_pair_ranks(Z, Z, 1.0, q, q.flip(0), node_filter=f),
        "score_pair_ranks_counted": lambda f: ops.score_pair_ranks_counted(Z, Z, 1.0, q, q.flip(0), node_filter=f),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="node filter of 3 nodes, tables of 6"):
            call(short)
        with pytest.raises(TypeError, match="ops.NodeFilter"):
            call(torch.tensor([0, 1, 0, 1, 0, 1]))
        if name in ("score_topk", "score_ranks"):                     # ordered scans take an asymmetric rule
            with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
                call(asym)
        else:
            with pytest.raises(ValueError, match="symmetric"):
                call(asym)
        with pytest.raises(ops._lib.DisenlinkHipError, match="no CPU fallback"):
            call(good)                                                # a good filter gets through to the device check


def _filtered_calls(lib, nf):
    """the four filtered entries with valid shapes and dummy non-NULL pointers: only the filter can be refused.  Nothing is
    launched: a refusal returns before the first launch, and n_queries = 0 / a short workspace end the good calls early."""
    p = C.c_void_p(256)
    return {
        "dl_score_topk_filtered": lambda: lib.dl_score_topk_filtered(p, p, 8, 2, 8, 1.0, p, 0, 4, None, None, 1, p, p, p, p, 0, None, nf),
        "dl_score_ranks_filtered": lambda: lib.dl_score_ranks_filtered(p, p, 8, 2, 8, 1.0, p, 0, p, p, 0, None, None, p, p, p, 0,
                                                                       None, nf),
        "dl_score_mine_filtered": lambda: lib.dl_score_mine_filtered(p, p, 8, 2, 8, 1.0, None, None, 0.0, 4, p, p, p, p, p, None, 0,
                                                                     None, nf),
        "dl_score_pair_ranks_filtered": lambda: lib.dl_score_pair_ranks_filtered(p, p, 8, 2, 8, 1.0, None, None, p, 1, p, p, p,
                                                                                 None, 0, None, nf),
    }


def test_c_abi_refuses_a_bad_filter():
    from disenlink_amd import _lib
    lib = _lib.load()
    p = 256
    for n_groups, group, allow, msg in ((0, p, p, b"n_groups=0 outside 1..64"), (65, p, p, b"n_groups=65 outside 1..64"),
                                        (-1, p, p, b"outside 1..64"), (2, None, p, b"NULL group or allow"),
                                        (2, p, None, b"NULL group or allow")):
        nf = C.byref(_lib.DlNodeFilter(group, n_groups, allow))
        for name, call in _filtered_calls(lib, nf).items():
            assert call() == -1, name                                 # DL_E_ARG
            assert msg in lib.dl_last_error(), (name, lib.dl_last_error())
    good = C.byref(_lib.DlNodeFilter(p, 64, p))
    for nf in (good, None):                                           # a good filter and NULL pass the filter check alike
        calls = _filtered_calls(lib, nf)
        assert calls["dl_score_topk_filtered"]() == 0                 # n_queries = 0: nothing to do
        assert calls["dl_score_ranks_filtered"]() == 0
        assert calls["dl_score_mine_filtered"]() == -3 and b"workspace too small" in lib.dl_last_error()
        assert calls["dl_score_pair_ranks_filtered"]() == -3 and b"workspace too small" in lib.dl_last_error()
    # the shape checks of the unfiltered entries come first, word for word
    assert lib.dl_score_mine_filtered(None, None, 8, 2, 8, 1.0, None, None, 0.0, 0, None, None, None, None, None, None, 0, None,
                                      good) == -1 and b"m=0 outside 1..65536" in lib.dl_last_error()


def test_header_and_binding_list_the_filtered_entries():
    import test_host_cpu
    from disenlink_amd import _lib
    names = test_host_cpu._declared_symbols()
    for n in ("dl_score_topk_filtered", "dl_score_ranks_filtered", "dl_score_mine_filtered", "dl_score_pair_ranks_filtered"):
        assert n in names and n in _lib.EXPORTS
        base = _lib.EXPORTS[n[:-len("_filtered")]]
        assert _lib.EXPORTS[n][0] is base[0] and _lib.EXPORTS[n][1][:-1] == base[1]       # the same arguments, then the filter
    test_host_cpu.test_library_exports_every_declared_symbol()


def test_cli_flag_errors(tmp_path):
    from disenlink_amd.main import main, load_node_groups
    groups = tmp_path / "groups.txt"
    groups.write_text("\n".join(str(i % 2) for i in range(10)) + "\n")
    base = ["--dataset", "squirrel", "--synthetic", "--epochs", "1", "--run", "1", "--quiet"]
    with pytest.raises(SystemExit, match="go together"):
        main(base + ["--mine", "5", "--node-groups", str(groups)])
    with pytest.raises(SystemExit, match="go together"):
        main(base + ["--mine", "5", "--link-rule", "same"])
    with pytest.raises(SystemExit, match="give one of them"):
        main(base + ["--node-groups", str(groups), "--link-rule", "different"])
    with pytest.raises(SystemExit):                                   # argparse: not a rule
        main(base + ["--mine", "5", "--node-groups", str(groups), "--link-rule", "other"])
    # the existing refusals keep their words and their precedence
    both = ["--node-groups", str(groups), "--link-rule", "same"]
    with pytest.raises(SystemExit, match="--mine M: 1 <= M <= 65536"):
        main(base + ["--mine", "70000"] + both)
    with pytest.raises(SystemExit, match="--mine runs on one GPU with fp32 tables only"):
        main(base + ["--mine", "5", "--table-dtype", "bf16"] + both)
    with pytest.raises(SystemExit, match="--rank-eval runs on one GPU only"):
        main(base + ["--rank-eval", "--gpus", "2"] + both)
    # the file: one integer per node
    f = load_node_groups(str(groups), 10, "different", "cpu")
    assert f.n_nodes == 10 and f.n_groups == 2 and f.allow.tolist() == [[False, True], [True, False]]
    npy = tmp_path / "groups.npy"
    np.save(npy, np.arange(10) % 3)
    assert load_node_groups(str(npy), 10, "same", "cpu").n_groups == 3
    with pytest.raises(SystemExit, match="one integer per node"):
        load_node_groups(str(groups), 11, "same", "cpu")
    with pytest.raises(SystemExit, match="outside 0..63"):
        np.save(npy, np.arange(10) * 10)
        load_node_groups(str(npy), 10, "same", "cpu")
    with pytest.raises(SystemExit, match="--node-groups"):
        load_node_groups(str(tmp_path / "missing.txt"), 10, "same", "cpu")
