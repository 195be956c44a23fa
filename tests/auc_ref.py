"""Plain reference of the tie-averaged AUC counts (dl_auc_pair_counts, metrics.AucPlan, metrics.auc_tie_avg) and the
cases the CPU and GPU tests share.  numpy only.

    u2(score, pos_idx, neg_idx) = 2 #{(p, n): s_n < s_p} + #{(p, n): s_n == s_p}     over ALL pairs, by comparison

— no sort, no search, no rank: fp32 values compared exactly (IEEE: -0.0 == +0.0, denormals are distinct values, +-inf
are equal to themselves), accumulated in int64, in chunks of the pair matrix.  AUC = u2 / (2 n_pos n_neg) as a double.
A NaN compares false with everything, so `u2` of a list that holds one is a number of no meaning: `has_nan` says so, and
the contract under test is that every form of the AUC returns NaN then.
"""
import numpy as np

PAIR_LIMIT = 7_000_000          # largest n_pos * n_neg of a case: the brute force stays a fraction of a second
CHUNK_PAIRS = 1 << 22           # pairs compared at a time


def u2(score, pos_idx, neg_idx) -> int:
    score = np.asarray(score)
    assert score.dtype == np.float32, score.dtype
    sp = score[np.asarray(pos_idx, dtype=np.int64)]
    sn = score[np.asarray(neg_idx, dtype=np.int64)]
    assert sp.size * sn.size <= PAIR_LIMIT, (sp.size, sn.size)
    total = 0
    rows = max(1, CHUNK_PAIRS // max(1, sn.size))
    for a in range(0, sp.size, rows):
        blk = sp[a:a + rows, None]
        total += 2 * int(np.count_nonzero(sn[None, :] < blk)) + int(np.count_nonzero(sn[None, :] == blk))
    return total


def auc(score, pos_idx, neg_idx) -> float:
    return u2(score, pos_idx, neg_idx) / (2.0 * float(len(pos_idx)) * float(len(neg_idx)))


def has_nan(score, pos_idx, neg_idx) -> bool:
    score = np.asarray(score)
    return bool(np.isnan(score[np.asarray(pos_idx, dtype=np.int64)]).any() or
                np.isnan(score[np.asarray(neg_idx, dtype=np.int64)]).any())


def index_lists(n_pos, n_neg, seed):
    """Two disjoint int64 index lists that cover range(n_pos + n_neg), interleaved and NOT sorted: a class is spread over
    the whole score vector and listed in a shuffled order, so a gather through the list is scattered."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_pos + n_neg).astype(np.int64)
    return perm[:n_pos].copy(), perm[n_pos:].copy()


def labels(n, pos_idx):
    y = np.zeros(n, np.float32)
    y[pos_idx] = 1.0
    return y


# ------------------------------------------------------------------------------------------------ the class-size ladder
N_SMALL = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)          # around the slice length of 1,024 and twice it
N_LARGE = (1023, 1024, 1025, 3001)                                     # plus n_small itself


def ladder_sizes():
    """(n_pos, n_neg) of every rung: each (n_small, n_large >= n_small) with the positives as the smaller class and with
    the negatives as the smaller class (equal sizes once)."""
    out = []
    for ns in N_SMALL:
        for nl in sorted({ns, *N_LARGE}):
            if nl >= ns:
                out.append((ns, nl))
                if nl != ns:
                    out.append((nl, ns))
    return out


def ladder_scores(n, seed):
    """Random scores: half of them on a grid of 64 levels in [0, 1] (ties inside and across the classes), half continuous
    logits of either sign."""
    rng = np.random.default_rng(seed)
    grid = (rng.integers(0, 65, n) / 64.0).astype(np.float32)
    cont = rng.standard_normal(n).astype(np.float32)
    return np.where(rng.random(n) < 0.5, grid, cont).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the score families
FAMILY_SIZES = ((65, 1025), (1025, 2049))                              # (n_small, n_large), used in both orientations
TINY = np.float32(1.17549435e-38)                                      # the smallest normal fp32


def _pick(rng, n, values):
    return np.asarray(values, dtype=np.float32)[rng.integers(0, len(values), n)]


def _three_levels(rng, n, pos_idx, neg_idx):
    return _pick(rng, n, [0.25, 0.5, 0.75])


def _all_equal(rng, n, pos_idx, neg_idx):
    return np.full(n, 0.625, np.float32)


def _huge_logits(rng, n, pos_idx, neg_idx):
    s = np.clip(rng.standard_normal(n) * 1e38, -3.3e38, 3.3e38).astype(np.float32)
    s[rng.random(n) < 0.2] = np.float32(3e38)
    s[rng.random(n) < 0.2] = np.float32(-3e38)
    s[rng.random(n) < 0.1] = np.float32(-2.5)
    return s


def _signed_zeros(rng, n, pos_idx, neg_idx):
    return _pick(rng, n, [0.0, -0.0, 0.0, -0.0, 1e-3, -1e-3])


def _denormals(rng, n, pos_idx, neg_idx):
    return _pick(rng, n, [1e-40, -1e-40, 1e-45, 0.0, TINY, -0.0, -1e-45, 2e-40])


def _plus_inf_in_the_sliced_class(rng, n, pos_idx, neg_idx):
    s = rng.standard_normal(n).astype(np.float32)
    small = pos_idx if len(pos_idx) <= len(neg_idx) else neg_idx
    large = neg_idx if small is pos_idx else pos_idx
    s[small[rng.random(len(small)) < 0.3]] = np.inf                    # next to the +inf padding of a ragged slice
    s[small[-1]] = np.inf                                              # ... and in its last real slot
    s[large[rng.random(len(large)) < 0.05]] = np.inf                   # searched +inf: ties with the real ones only
    return s


def _minus_inf_in_both(rng, n, pos_idx, neg_idx):
    s = rng.standard_normal(n).astype(np.float32)
    s[rng.random(n) < 0.25] = -np.inf
    s[pos_idx[0]] = -np.inf
    s[neg_idx[0]] = -np.inf
    return s


def _only_infinities(rng, n, pos_idx, neg_idx):
    return _pick(rng, n, [np.inf, -np.inf])


def _positives_above(rng, n, pos_idx, neg_idx):                        # AUC exactly 1
    s = rng.random(n).astype(np.float32)
    s[pos_idx] += np.float32(2.0)
    return s


def _positives_below(rng, n, pos_idx, neg_idx):                        # AUC exactly 0
    s = rng.random(n).astype(np.float32)
    s[pos_idx] -= np.float32(2.0)
    return s


FAMILIES = {
    "three_levels": _three_levels, "all_equal": _all_equal, "huge_logits": _huge_logits, "signed_zeros": _signed_zeros,
    "denormals": _denormals, "plus_inf_sliced": _plus_inf_in_the_sliced_class, "minus_inf_both": _minus_inf_in_both,
    "only_inf": _only_infinities, "separated_1": _positives_above, "separated_0": _positives_below,
}
EXACT_AUC = {"all_equal": 0.5, "separated_1": 1.0, "separated_0": 0.0}


def family_sizes():
    return [s for a, b in FAMILY_SIZES for s in ((a, b), (b, a))]


class Case:
    """One input: `score` (fp32), the two index lists, and the reference count (formed on first use, then kept)."""

    def __init__(self, name, score, pos_idx, neg_idx):
        self.name, self.score, self.pos_idx, self.neg_idx = name, score, pos_idx, neg_idx
        self.n_pos, self.n_neg = len(pos_idx), len(neg_idx)
        self._u2 = None
        for a in (score, pos_idx, neg_idx):
            a.setflags(write=False)

    @property
    def u2(self) -> int:
        if self._u2 is None:
            self._u2 = u2(self.score, self.pos_idx, self.neg_idx)
        return self._u2

    @property
    def auc(self) -> float:
        return self.u2 / (2.0 * float(self.n_pos) * float(self.n_neg))

    @property
    def label(self):
        return labels(self.score.size, self.pos_idx)


def ladder_case(n_pos, n_neg) -> Case:
    seed = 1000003 * n_pos + n_neg
    pos_idx, neg_idx = index_lists(n_pos, n_neg, seed)
    return Case(f"ladder_{n_pos}x{n_neg}", ladder_scores(n_pos + n_neg, seed + 1), pos_idx, neg_idx)


def family_case(family, n_pos, n_neg) -> Case:
    seed = 7 * n_pos + 13 * n_neg + sorted(FAMILIES).index(family)
    pos_idx, neg_idx = index_lists(n_pos, n_neg, seed)
    score = FAMILIES[family](np.random.default_rng(seed + 1), n_pos + n_neg, pos_idx, neg_idx).astype(np.float32)
    return Case(f"{family}_{n_pos}x{n_neg}", score, pos_idx, neg_idx)


_CASES = {}


def case(kind, *args) -> Case:
    """ladder_case / family_case, built once per process and shared by the tests (the arrays are read-only)."""
    key = (kind, *args)
    if key not in _CASES:
        _CASES[key] = ladder_case(*args) if kind == "ladder" else family_case(*args)
    return _CASES[key]


def all_case_keys():
    return [("ladder", a, b) for a, b in ladder_sizes()] + [("family", f, a, b) for f in FAMILIES for a, b in family_sizes()]


# ------------------------------------------------------------------------------------------------ NaN placements
def nan_inputs(n_pos, n_neg, seed=5):
    """The five NaN inputs of the contract on a NaN-free base: {name: (score, pos_idx, neg_idx)}.  Every one must give a
    NaN AUC, whichever class is the smaller one."""
    pos_idx, neg_idx = index_lists(n_pos, n_neg, seed)
    base = ladder_scores(n_pos + n_neg, seed + 1)
    out = {}

    def put(name, where):
        s = base.copy()
        s[where] = np.nan
        out[name] = (s, pos_idx, neg_idx)
    put("one_nan_positive", pos_idx[n_pos // 2])
    put("one_nan_negative", neg_idx[n_neg // 2])
    put("all_nan", np.arange(n_pos + n_neg))
    put("every_positive_nan", pos_idx)
    put("every_negative_nan", neg_idx)
    return out
