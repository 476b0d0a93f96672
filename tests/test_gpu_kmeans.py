"""GPU: the device k-means of csrc/kmeans.hip (miclip_kmeans_seed, miclip_kmeans_lloyd)
through the raw C ABI, and compute_prototypes(kmeans="device") on top of it.

The yardstick is tests/_kmeans_ref.py (float64; tests/test_kmeans_ref.py holds it against
scikit-learn). Every output sits in front of canary elements, which must stay untouched,
and every float input in front of NaNs, which must never be read.

Labels: with g = 4 (D + 8) 2^-23, a row whose float64 gap (second-nearest minus nearest
d^2) exceeds g must carry the float64 label; a row inside g may carry either of its two
nearest centres. The fixed seeds keep at most 5 % of a one-step case's rows inside g and
every trajectory's smallest gap at 1e-3 or more; both preconditions are asserted.

Bars: 4 x the largest error measured on the MI355X over the one-step cases of this file
(every test prints its figures before it asserts), never above the derived cap:
  centres against the float64 means of the kernel's own labels, in units of max|x|,
      cap (largest cluster + 8) 2^-24: measured 4.60e-7 (n = 1100, D = 1024)
  inertia against float64 on the kernel's own labels and centres,
      cap (D + 8) 2^-23 relative: measured 1.76e-7 (n = 1100, D = 1024)
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import _kmeans_ref as K

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, PAD = -7.0, -7, 8
SLOTS = 16
MEASURED_CENTRE = 4.60e-7
MEASURED_INERTIA = 1.76e-7


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan_padded(a):
    """Device fp32 copy of `a` with PAD NaNs behind it (flat)."""
    flat = np.concatenate([np.ascontiguousarray(a, np.float32).ravel(),
                           np.full(PAD, np.nan, np.float32)])
    return torch.from_numpy(flat).cuda()


def _canary(n, dtype):
    return torch.full((n + PAD,), CANARY_I if dtype == torch.int32 else CANARY_F, device="cuda",
                      dtype=dtype)


def _take(t, n):
    a = t.cpu().numpy()
    assert (a[n:] == (CANARY_I if a.dtype == np.int32 else CANARY_F)).all(), "canary written"
    return a[:n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def label_gap_bar(D):
    return 4.0 * (D + 8) * 2.0 ** -23


def centre_bar(n_max, xmax):
    return min(4.0 * MEASURED_CENTRE, (n_max + 8) * 2.0 ** -24) * xmax


def inertia_bar(D):
    return min(4.0 * MEASURED_INERTIA, (D + 8) * 2.0 ** -23)


class Launch:
    """One set of problems on one data set. `inv` gives each row's class; problems is a
    list of (class, k). Buffers are padded as the module docstring says."""

    def __init__(self, x, inv, problems):
        from miclip import outliers as O
        self.O = O
        self.x = np.ascontiguousarray(x, np.float32)
        self.N, self.D = self.x.shape
        self.inv = np.asarray(inv, np.int64)
        ncls = int(self.inv.max()) + 1
        self.order = np.argsort(self.inv, kind="stable").astype(np.int32)
        self.counts = np.bincount(self.inv, minlength=ncls)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.problems = list(problems)
        self.table = O._kmeans_table(self.counts, [c for c, _ in problems],
                                     [k for _, k in problems], 1, "cuda")
        self.Pn = len(problems)
        self.xd = _nan_padded(self.x)
        self.layout = {"order": torch.from_numpy(self.order).cuda(),
                       "offsets": torch.from_numpy(self.offsets).cuda()}
        self.off = np.concatenate([[0], np.cumsum([self.counts[c] for c, _ in problems])])
        self.total = int(self.off[-1])

    def rows(self, p):
        """The data rows of problem p, in class order (float32)."""
        c = self.problems[p][0]
        return self.x[self.order[self.offsets[c]:self.offsets[c + 1]]]

    def _args(self):
        from miclip import _lib
        lib = _lib.load_library()
        t, L = self.table, self.layout
        head = (_ptr(self.xd), _ptr(L["order"]), _ptr(L["offsets"]), self.D, _ptr(t["cls"]),
                _ptr(t["k"]), _ptr(t["off"]), self.Pn, t["k_max"])
        return _lib, lib, head

    def seed(self, u):
        """u [Pn, 16] -> (picks [Pn, 16], centres [Pn, 16, D]); unwritten slots keep the canary."""
        _lib, lib, head = self._args()
        ud = _nan_padded(u)
        scratch = _canary(self.total, torch.float32)
        picks = _canary(self.Pn * SLOTS, torch.int32)
        cen = _canary(self.Pn * SLOTS * self.D, torch.float32)
        _lib.check(lib.miclip_kmeans_seed(*head, _ptr(ud), _ptr(scratch), _ptr(picks), _ptr(cen),
                                          _lib.stream_handle()), "miclip_kmeans_seed")
        torch.cuda.synchronize()
        _take(scratch, self.total)
        return (_take(picks, self.Pn * SLOTS).reshape(self.Pn, SLOTS),
                _take(cen, self.Pn * SLOTS * self.D).reshape(self.Pn, SLOTS, self.D))

    def lloyd(self, c0, max_iter, tol):
        """c0: list of [k, D] initial centres per problem; tol [Pn]. Returns a dict of numpy
        arrays; centre slots >= k must come back as the canary they went in with."""
        _lib, lib, head = self._args()
        cen_h = np.full((self.Pn, SLOTS, self.D), CANARY_F, np.float32)
        for p, c in enumerate(c0):
            cen_h[p, :len(c)] = c
        cen = torch.from_numpy(np.concatenate([cen_h.ravel(),
                                               np.full(PAD, CANARY_F, np.float32)])).cuda()
        told = _nan_padded(tol)
        scratch = _canary(self.total, torch.float32)
        labels = _canary(self.total, torch.int32)
        inertia = _canary(self.Pn, torch.float32)
        n_iter = _canary(self.Pn, torch.int32)
        strict = _canary(self.Pn, torch.int32)
        counts = _canary(self.Pn * SLOTS, torch.int32)
        _lib.check(lib.miclip_kmeans_lloyd(*head, _ptr(told), int(max_iter), _ptr(scratch),
                                           _ptr(cen), _ptr(labels), _ptr(inertia), _ptr(n_iter),
                                           _ptr(strict), _ptr(counts), _lib.stream_handle()),
                   "miclip_kmeans_lloyd")
        torch.cuda.synchronize()
        _take(scratch, self.total)
        out_c = _take(cen, self.Pn * SLOTS * self.D).reshape(self.Pn, SLOTS, self.D)
        for p, (_, k) in enumerate(self.problems):
            assert (out_c[p, k:] == CANARY_F).all(), "centre slot >= k written"
        lab = _take(labels, self.total)
        return {"centres": out_c, "labels": [lab[self.off[p]:self.off[p + 1]]
                                             for p in range(self.Pn)],
                "inertia": _take(inertia, self.Pn), "n_iter": _take(n_iter, self.Pn),
                "strict": _take(strict, self.Pn),
                "counts": _take(counts, self.Pn * SLOTS).reshape(self.Pn, SLOTS)}


def _check_labels(lab, x, centres64, D, what, max_inside=None):
    """The label bar of the module docstring against float64 centres."""
    want, _, gap, second = K.assign(x, centres64)
    g = label_gap_bar(D)
    inside = gap <= g
    if max_inside is not None:
        assert inside.mean() <= max_inside, f"{what}: {inside.mean():.3f} of the rows inside g"
    assert np.array_equal(lab[~inside], want[~inside]), what
    assert ((lab[inside] == want[inside]) | (lab[inside] == second[inside])).all(), what
    return int(inside.sum())


def _check_numbers(out, p, x, k, D, what):
    """Centres against the float64 means of the kernel's own labels, inertia against float64
    on the kernel's own labels and centres, counts against a bincount. Returns the figures."""
    lab = out["labels"][p]
    assert lab.min() >= 0 and lab.max() < k
    cnt = np.bincount(lab, minlength=k)
    assert np.array_equal(out["counts"][p, :k], cnt) and (out["counts"][p, k:] == 0).all()
    assert (cnt > 0).all(), f"{what}: an empty cluster in a case built to have none"
    x64 = x.astype(np.float64)
    means = np.stack([x64[lab == j].mean(axis=0) for j in range(k)])
    got = out["centres"][p, :k].astype(np.float64)
    dc = float(np.abs(got - means).max())
    want_i = float(((x64 - got[lab]) ** 2).sum())
    di = abs(float(out["inertia"][p]) - want_i) / max(want_i, 1e-300) if want_i > 0 else \
        abs(float(out["inertia"][p]))
    xmax = float(np.abs(x).max())
    print(f"{what}: centres / max|x| {dc / xmax:.3e} (cap {(cnt.max() + 8) * 2.0 ** -24:.3e}) "
          f"inertia rel {di:.3e} (cap {(D + 8) * 2.0 ** -23:.3e})")
    assert dc <= centre_bar(int(cnt.max()), float(np.abs(x).max())), what
    assert di <= inertia_bar(D), what
    return dc, di


# ------------------------------------------------------------------ a. one step
def _modes_case(n, D, k, seed):
    """n planted rows in k modes (D = 1: k well separated values) and one row of each mode
    as the initial centres, so that the labelling is already stable after one step."""
    if D == 1:
        rng = np.random.default_rng(seed)
        mode = rng.permutation(np.arange(n) % k)
        x = (3.0 * mode + rng.uniform(-0.4, 0.4, n))[:, None].astype(np.float32)
    else:
        x, mode = K.planted(n, D, k, seed)
    c0 = np.stack([x[np.flatnonzero(mode == j)[0]] for j in range(k)])
    return x, c0


ONE_STEP = [(2, 1, 2), (15, 16, 2), (17, 48, 16), (33, 130, 3), (300, 768, 6), (1100, 1024, 5)]


@pytest.mark.parametrize("n,D,k", ONE_STEP)
def test_one_step_against_fp64(n, D, k):
    """max_iter = 1 from given centres; a second, smaller class with another k shares the
    launch, and the two classes' rows are interleaved in memory."""
    k2 = 3 if k == 2 else 2
    xa, ca = _modes_case(n, D, k, seed=11)
    xb, cb = _modes_case(12, D, k2, seed=12)
    rng = np.random.default_rng(5)
    inv = rng.permutation(np.r_[np.zeros(n, np.int64), np.ones(12, np.int64)])
    x = np.empty((n + 12, D), np.float32)
    x[inv == 0], x[inv == 1] = xa, xb
    L = Launch(x, inv, [(0, k), (1, k2)])
    tol = np.asarray([K.tol_of(xa), K.tol_of(xb)], np.float32)
    out = L.lloyd([ca, cb], 1, tol)
    for p, (xs, c0, kk) in enumerate(((xa, ca, k), (xb, cb, k2))):
        what = f"one step n={len(xs)} D={D} k={kk}"
        assert np.array_equal(L.rows(p), xs)
        fit = K.lloyd(xs, c0, 1, float(tol[p]))
        first, _, _, _ = K.assign(xs, c0)
        assert np.array_equal(first, fit.labels), "precondition: the labelling is stable"
        assert out["n_iter"][p] == 1 and out["strict"][p] == 0
        _check_labels(out["labels"][p], xs, fit.centres, D, what, max_inside=0.05)
        _check_numbers(out, p, xs, kk, D, what)


# ------------------------------------------------------------------ b. trajectories
# seeds fixed on the CPU so that the yardstick's smallest gap over the trajectory is >= 1e-3
TRAJ = [(33, 17, 3), (60, 16, 2), (240, 96, 4), (600, 130, 6)]
TRAJ_SEED = {  # (n, D, k, init) -> seed; the yardstick's smallest gap and n_iter with it
    (33, 17, 3, "rows"): 1,        # 4.3e-3, 3
    (33, 17, 3, "empty"): 1,       # 3.6e-1, 3
    (60, 16, 2, "rows"): 47,       # 2.2e-3, 3
    (60, 16, 2, "empty"): 0,       # 2.8e-1, 3
    (240, 96, 4, "rows"): 131,     # 1.5e-3, 3
    (240, 96, 4, "empty"): 0,      # 2.4e-1, 3
    (600, 130, 6, "rows"): 106,    # 1.7, 2
    (600, 130, 6, "empty"): 16,    # 4.8e-2, 3
}


def _traj_case(n, D, k, init, seed):
    x, _ = K.planted(n, D, k, seed)
    rng = np.random.default_rng(seed + 1)
    c0 = x[rng.choice(n, k, replace=False)].copy()
    if init == "empty":
        c0[k - 1] = -3.0 * x[0]          # farther from every row than any other centre
    return x, c0


@pytest.mark.parametrize("init", ["rows", "empty"])
@pytest.mark.parametrize("n,D,k", TRAJ)
def test_trajectory_equals_yardstick(n, D, k, init):
    x, c0 = _traj_case(n, D, k, init, TRAJ_SEED[(n, D, k, init)])
    tol = K.tol_of(x)
    fit = K.lloyd(x, c0, 100, tol)
    assert fit.min_gap >= 1e-3, f"precondition: smallest gap {fit.min_gap:.2e}"
    if init == "empty":
        assert fit.relocated >= 1, "precondition: no cluster was emptied"
    L = Launch(x, np.zeros(n, np.int64), [(0, k)])
    out = L.lloyd([c0], 100, np.asarray([tol], np.float32))
    what = f"trajectory n={n} D={D} k={k} {init}"
    print(f"{what}: n_iter {out['n_iter'][0]} (yardstick {fit.n_iter}) strict {out['strict'][0]} "
          f"(yardstick {int(fit.strict)}) min gap {fit.min_gap:.2e} relocated {fit.relocated}")
    assert np.array_equal(out["labels"][0], fit.labels)
    assert out["n_iter"][0] == fit.n_iter and out["strict"][0] == int(fit.strict)
    cnt = np.bincount(fit.labels, minlength=k)
    dc = float(np.abs(out["centres"][0, :k] - fit.centres).max())
    print(f"{what}: centres against the yardstick {dc:.3e}")
    assert dc <= centre_bar(int(cnt.max()), float(np.abs(x).max()))
    _check_numbers(out, 0, x, k, D, what)


MAXITER2_SEED = (33, 17, 3, 83)   # fixed on the CPU: stops non-strict at max_iter = 2, gap 2.5e-3


def test_max_iter_2_non_strict_labels_match_centres():
    n, D, k, seed = MAXITER2_SEED
    x, c0 = _traj_case(n, D, k, "rows", seed)
    tol = K.tol_of(x)
    fit = K.lloyd(x, c0, 2, tol)
    assert not fit.strict and fit.n_iter == 2, "precondition: a non-strict stop at max_iter"
    assert fit.min_gap >= 1e-3, f"precondition: smallest gap {fit.min_gap:.2e}"
    L = Launch(x, np.zeros(n, np.int64), [(0, k)])
    out = L.lloyd([c0], 2, np.asarray([tol], np.float32))
    assert out["n_iter"][0] == 2 and out["strict"][0] == 0
    assert np.array_equal(out["labels"][0], fit.labels)
    # the returned labels are the assignment to the RETURNED centres, not to the previous ones
    _check_labels(out["labels"][0], x, out["centres"][0, :k].astype(np.float64), D, "max_iter 2")
    before = K.lloyd(x, c0, 1, -1.0)          # centres after one iteration
    prev, _, _, _ = K.assign(x, before.centres)
    assert not np.array_equal(prev, fit.labels), "precondition: the last E-step moved a row"


# ------------------------------------------------------------------ c. ties
def test_identical_initial_centres_lower_index_takes_every_row():
    """c_0 == c_1: every distance ties, index 0 takes all rows, cluster 1 is empty and is
    re-seeded with the row farthest from c_0 (bit for bit that row)."""
    n, D = 40, 24
    x, _ = K.planted(n, D, 2, seed=3)
    c0 = np.stack([x[5], x[5]])
    own = K.sqdist(x, c0[:1])[:, 0]
    far = int(np.argmax(own))
    assert np.sort(own)[-1] - np.sort(own)[-2] > 1e-3, "precondition: one farthest row"
    L = Launch(x, np.zeros(n, np.int64), [(0, 2)])
    out = L.lloyd([c0], 1, np.asarray([0.0], np.float32))
    fit = K.lloyd(x, c0, 1, 0.0)
    assert fit.relocated == 1
    assert np.array_equal(_bits(out["centres"][0, 1]), _bits(x[far]))
    rest = np.delete(x.astype(np.float64), far, axis=0).mean(axis=0)
    assert np.abs(out["centres"][0, 0] - rest).max() <= centre_bar(n, float(np.abs(x).max()))
    assert np.abs(out["centres"][0, :2] - fit.centres).max() <= centre_bar(n, float(np.abs(x).max()))
    _check_labels(out["labels"][0], x, fit.centres, D, "identical centres")


def test_exactly_equal_distances_go_to_the_lowest_index():
    """Duplicate rows at exactly equal distance from two or three centres (all numbers are
    exact in fp32): the first E-step gives them to the lowest index, which the centres of
    max_iter = 1 show."""
    D = 16
    e = np.eye(D, dtype=np.float32)
    c0 = np.stack([e[0], e[1], e[2]])
    x = np.concatenate([np.tile(e[3], (5, 1)),                  # ties 0 / 1 / 2 -> 0
                        np.tile(0.5 * (e[1] + e[2]), (4, 1)),   # ties 1 / 2 -> 1
                        np.tile(e[2], (3, 1)), np.tile(e[0], (2, 1))])
    first, _, gap, _ = K.assign(x, c0)
    assert (gap[:9] == 0).all() and (first[:5] == 0).all() and (first[5:9] == 1).all()
    L = Launch(x, np.zeros(len(x), np.int64), [(0, 3)])
    out = L.lloyd([c0], 1, np.asarray([0.0], np.float32))
    fit = K.lloyd(x, c0, 1, 0.0)
    e64 = np.eye(D)
    want = np.stack([(5 * e64[3] + 2 * e64[0]) / 7, 0.5 * (e64[1] + e64[2]), e64[2]])
    assert np.abs(fit.centres - want).max() < 1e-15
    assert np.abs(out["centres"][0, :3] - want).max() <= 2.0 ** -23
    assert np.array_equal(out["labels"][0], fit.labels)


# ------------------------------------------------------------------ d. seeding
def _uniforms(Pn, seed):
    return np.random.default_rng(seed).random((Pn, SLOTS), dtype=np.float32)


@pytest.mark.parametrize("n,D,k", [(2, 1, 2), (33, 17, 3), (257, 48, 16), (300, 130, 6)])
def test_seeding_on_the_kernels_own_picks(n, D, k):
    x, _ = _modes_case(n, D, min(k, 6), seed=21)
    L = Launch(x, np.zeros(n, np.int64), [(0, k), (0, k)])
    u = _uniforms(2, seed=n)
    picks, cen = L.seed(u)
    x64 = x.astype(np.float64)
    for p in range(2):
        pk = picks[p, :k]
        assert (picks[p, k:] == CANARY_I).all() and (cen[p, k:] == CANARY_F).all()
        assert pk.min() >= 0 and pk.max() < n and len(set(pk.tolist())) == k
        assert pk[0] == K.first_pick(u[p, 0], n)
        assert np.array_equal(_bits(cen[p, :k]), _bits(x[pk]))
        for t in range(1, k):
            mind = K.seed_mind(x64, pk[:t])
            cum = np.cumsum(mind)
            total = cum[-1]
            tau = (n + D + 8) * 2.0 ** -23 * total
            s = int(pk[t])
            target = np.float64(u[p, t]) * total
            lo = cum[s - 1] if s > 0 else 0.0
            assert mind[s] > 0
            assert lo - tau <= target <= cum[s] + tau, (p, t, s, lo, target, cum[s], tau)


def test_seeding_duplicate_points_returns_the_distinct_points():
    k, D = 5, 12
    pts = np.random.default_rng(2).standard_normal((k, D)).astype(np.float32)
    which = np.random.default_rng(3).permutation(np.arange(60) % k)
    x = pts[which]
    L = Launch(x, np.zeros(len(x), np.int64), [(0, k)] * 4)
    picks, cen = L.seed(_uniforms(4, seed=9))
    for p in range(4):
        assert sorted(which[picks[p, :k]].tolist()) == list(range(k))
        assert np.array_equal(_bits(cen[p, :k]), _bits(x[picks[p, :k]]))


def test_seeding_zero_total_picks_the_lowest_free_rows():
    k, D, n = 4, 20, 9
    x = np.tile(np.random.default_rng(4).standard_normal((1, D)).astype(np.float32), (n, 1))
    u = _uniforms(2, seed=1)
    u[:, 0] = [0.0, 0.3]                     # pick 0 = row 0 / row 2
    L = Launch(x, np.zeros(n, np.int64), [(0, k)] * 2)
    picks, _ = L.seed(u)
    assert picks[0, :k].tolist() == [0, 1, 2, 3]
    assert picks[1, :k].tolist() == [2, 0, 1, 3]


# ------------------------------------------------------------------ e. invariance
def test_result_does_not_depend_on_the_launch_and_repeats_bit_for_bit():
    """Seed + Lloyd of one problem alone, and inside a 9-problem launch at index 0, 4, 8."""
    rng = np.random.default_rng(8)
    xa, _ = K.planted(150, 80, 4, seed=31)
    xb, _ = K.planted(70, 80, 3, seed=32)
    inv = rng.permutation(np.r_[np.zeros(150, np.int64), np.ones(70, np.int64)])
    x = np.empty((220, 80), np.float32)
    x[inv == 0], x[inv == 1] = xa, xb
    mine, other = (0, 4), [(1, 3), (0, 2), (1, 2), (0, 5), (1, 4), (0, 3), (1, 2), (0, 6)]
    u_mine, u_other = _uniforms(1, seed=40), _uniforms(8, seed=41)
    tol_c = [K.tol_of(xa), K.tol_of(xb)]

    def run(problems, u):
        L = Launch(x, inv, problems)
        picks, cen = L.seed(u)
        c0 = [cen[p, :k] for p, (_, k) in enumerate(problems)]
        out = L.lloyd(c0, 100, np.asarray([tol_c[c] for c, _ in problems], np.float32))
        out["picks"] = picks
        return out

    def same(a, pa, b, pb):
        k = mine[1]
        for key in ("picks", "counts"):
            assert np.array_equal(a[key][pa], b[key][pb]), key
        for key in ("inertia", "n_iter", "strict"):
            assert _bits(a[key][pa:pa + 1]) == _bits(b[key][pb:pb + 1]), key
        assert np.array_equal(_bits(a["centres"][pa, :k]), _bits(b["centres"][pb, :k]))
        assert np.array_equal(a["labels"][pa], b["labels"][pb])

    alone = run([mine], u_mine)
    same(alone, 0, run([mine], u_mine), 0)
    for at in (0, 4, 8):
        problems = other[:at] + [mine] + other[at:]
        u = np.concatenate([u_other[:at], u_mine, u_other[at:]])
        same(alone, 0, run(problems, u), at)


# ------------------------------------------------------------------ f. the scorer
D_SCORER = 96
TOL_SIM = 5e-6          # tests/test_outliers.py


def _planted_cache():
    """3 classes at D = 96: 60 rows in 3 modes, 15 rows in 1 mode (k = 1), 120 rows in 4."""
    xs, labs, modes = [], [], []
    for label, (n, k) in zip((3, 5, 9), ((60, 3), (15, 1), (120, 4))):
        x, mode = K.planted(n, D_SCORER, k, seed=50 + label)
        xs.append(x)
        labs.append(np.full(n, label))
        modes.append(mode)
    perm = np.random.default_rng(6).permutation(sum(len(x) for x in xs))
    x, lab, mode = np.concatenate(xs)[perm], np.concatenate(labs)[perm], np.concatenate(modes)[perm]
    meta = pd.DataFrame({"file_name": [f"f{i:04d}.jpg" for i in range(len(x))],
                         "ground_truth_num_label": lab})
    return x, lab, mode, meta


def _partition_of(scorer, res, lab, label):
    """Per row of class `label`: the prototype it is nearest to (cosine), on the host."""
    rows = scorer.embeddings.cpu().numpy()[lab == label].astype(np.float64)
    protos = res.prototypes[label].cpu().numpy().astype(np.float64)
    return np.argmax(rows @ protos.T, axis=1)


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_scorer_device_backend_finds_the_planted_partition():
    from miclip.outliers import MultiPrototypeScorer
    x, lab, mode, meta = _planted_cache()
    frames, results = {}, {}
    for backend in ("sklearn", "device"):
        sc = MultiPrototypeScorer(torch.from_numpy(x), torch.from_numpy(lab), meta)
        res = sc.compute_prototypes(kmeans=backend)
        assert sc._prototype_config[-1] == backend
        assert res.k_per_class == {3: 3, 5: 1, 9: 4}
        for label in (3, 5, 9):
            part = _partition_of(sc, res, lab, label)
            assert _same_partition(part, mode[lab == label]), (backend, label)
            assert sorted(res.prototype_counts[label]) == sorted(
                np.bincount(mode[lab == label]).tolist()), (backend, label)
        frames[backend], results[backend] = sc.score_prototype_distance(), res
    a = frames["sklearn"].set_index("file_name")
    b = frames["device"].set_index("file_name").loc[a.index]
    for col in ("sim_to_prototype", "outlier_score", "sim_to_other_class_best",
                "margin_to_other_class"):
        d = float(np.abs(a[col].to_numpy(np.float64) - b[col].to_numpy(np.float64)).max())
        print(f"planted cache {col}: device against sklearn backend {d:.3e}")
        assert d <= TOL_SIM, col
    # prototypes matched by nearest: the same vectors up to the order inside a class
    for label in (3, 9):
        pa = results["sklearn"].prototypes[label].cpu().numpy()
        pb = results["device"].prototypes[label].cpu().numpy()
        match = np.argmax(pa @ pb.T, axis=1)
        assert sorted(match.tolist()) == list(range(len(pa)))
        assert np.abs(pa - pb[match]).max() <= TOL_SIM
        assert np.array_equal(a.loc[a.ground_truth_num_label == label, "prototype_size"].to_numpy(),
                              b.loc[b.ground_truth_num_label == label, "prototype_size"].to_numpy())


def test_scorer_on_the_golden_cache_takes_the_first_best_restart():
    import os
    from conftest import GOLDEN
    from miclip.outliers import MultiPrototypeScorer
    from sklearn.cluster import KMeans
    z = np.load(os.path.join(GOLDEN, "outliers.npz"))
    emb, lab = z["emb"].astype(np.float32), z["labels"]
    meta = pd.DataFrame({"file_name": z["meta_file_name"], "ground_truth_num_label": lab})
    sc = MultiPrototypeScorer(torch.from_numpy(emb), torch.from_numpy(lab), meta)
    res = sc.compute_prototypes(kmeans="device")
    fit = sc._kmeans_fit
    inertia = fit["inertia"].cpu().numpy()
    chosen = fit["chosen"].cpu().numpy()
    assert inertia.shape[1] == 10 and np.isfinite(inertia).all()
    assert np.array_equal(chosen, np.argmin(inertia, axis=1))       # numpy: the first minimum
    assert (fit["n_iter"].cpu().numpy() >= 1).all()
    for label, n_c in res.class_counts.items():
        assert sum(res.prototype_counts[label]) == n_c == int((lab == label).sum())
        assert len(res.prototype_counts[label]) == res.k_per_class[label]
    xn = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    for i, label in enumerate(fit["classes"]):
        k = res.k_per_class[label]
        km = KMeans(n_clusters=k, random_state=0, n_init=10, max_iter=100).fit(xn[lab == label])
        print(f"golden cache class {label} (n={int((lab == label).sum())}, k={k}): inertia device / "
              f"sklearn = {inertia[i, chosen[i]] / km.inertia_:.4f}")


def test_scorer_input_validation():
    from miclip.outliers import MultiPrototypeScorer
    x, lab, _, meta = _planted_cache()
    sc = MultiPrototypeScorer(torch.from_numpy(x), torch.from_numpy(lab), meta)
    with pytest.raises(ValueError, match="bogus"):
        sc.compute_prototypes(kmeans="bogus")
    with pytest.raises(ValueError, match="16"):
        sc.compute_prototypes(k_mode="fixed", k_fixed=17, k_max=17, min_samples_per_proto=1,
                              kmeans="device")
