"""GPU: edge cases of the outlier-scoring ops (csrc/scoring.hip: row_norms, div_rows,
class_sums, centroid, proto_score) through miclip.outliers' helpers and, where a canary
or the `sums` buffer is needed, the raw C ABI.

What is compared with what (the yardstick is tests/_head_ref.py):
  * row norms / normalised rows against float64, at D below, on and off the 64- and
    256-wide strides; a zero row gives norm 0 and zeros;
  * class sums bit for bit against a strict sequential fp32 accumulation in ascending
    sample order (a numpy float32 loop), class sizes on both sides of the unroll of 8,
    interleaved labels, ragged 64-column blocks, an empty class;
  * proto_scores' integer and best-value outputs exactly against numpy on the kernel's
    OWN similarity matrix, which is assembled from single-prototype launches (a column
    of the matrix is an independent ascending-k fmaf chain, shown by
    test_similarity_is_independent_of_the_tile_position), with the first index on ties;
    that matrix against float64.
Every output has canary elements behind it, which must stay untouched.

Bars: 4 x the largest error measured on the MI355X over the cases of this file (every
test prints its figure before it asserts), never above the cap next to it.
  row norms, relative, cap (D / 64 + 8) * 2^-23: 7.37e-8
  normalised rows, relative to the row's largest element, same cap: 9.88e-8
  centroids against fp64 normalize(mean), cap 2e-6 (TOL_VEC): 4.41e-8
  similarities of unit-norm rows against fp64, cap 5e-6 (TOL_SIM): 2.27e-7
  cosine with inv_nx / inv_np given, cap 5e-6: 1.57e-7
"""
import ctypes

import numpy as np
import pytest
import torch

import _head_ref as R

pytestmark = pytest.mark.gpu

TOL_SIM, TOL_VEC = 5e-6, 2e-6       # tests/test_outliers.py
EPS = 1e-12
CANARY_F, CANARY_I, PAD = -7.0, -7, 8

MEASURED_NORM = 7.37e-8
MEASURED_DIV = 9.88e-8
MEASURED_CENT = 4.41e-8
MEASURED_SIM = 2.27e-7
MEASURED_COS = 1.57e-7


def _bar(measured, cap):
    """4 x measured, never above the cap."""
    return min(4.0 * measured, cap)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def _padded(n, dtype=torch.float32):
    """n elements + PAD canaries."""
    return torch.full((n + PAD,), CANARY_I if dtype == torch.int32 else CANARY_F, device="cuda",
                      dtype=dtype)


def _take(t, n):
    a = t.cpu().numpy()
    assert (a[n:] == (CANARY_I if a.dtype == np.int32 else CANARY_F)).all(), "canary written"
    return a[:n]


# ------------------------------------------------------------------ a. row_norms / div_rows
def _row_norms_raw(x, eps=EPS):
    from miclip import _lib
    lib = _lib.load_library()
    N, D = x.shape
    xd = _dev(x)
    norms, out = _padded(N), _padded(N * D)
    _lib.check(lib.miclip_row_norms(_ptr(xd), N, D, _ptr(norms), eps, _ptr(out),
                                    _lib.stream_handle()), "miclip_row_norms")
    return _take(norms, N), _take(out, N * D).reshape(N, D)


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 257, 1000])
def test_row_norms_and_div_rows_against_fp64(N, D):
    from miclip.outliers import _row_norms
    rng = np.random.default_rng(100 * D + N)
    x = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-3, 3, (N, 1)))).astype(np.float32)
    if N > 1:
        x[2] = 0.0                      # a zero row among the others
    norms, out = _row_norms_raw(x)
    want_n, want_o = R.row_norms(x), R.div_rows(x, EPS)
    nz = want_n > 0
    e_n = float((np.abs(norms - want_n)[nz] / want_n[nz]).max())
    e_o = float((np.abs(out - want_o).max(axis=1)[nz] / np.abs(want_o).max(axis=1)[nz]).max())
    cap = (D / 64 + 8) * 2.0 ** -23
    bar_n, bar_o = _bar(MEASURED_NORM, cap), _bar(MEASURED_DIV, cap)
    print(f"N={N} D={D}: norm rel err {e_n:.3g} (bar {bar_n:.3g}), row rel err {e_o:.3g} "
          f"(bar {bar_o:.3g}), cap {cap:.3g}")
    assert e_n <= bar_n and e_o <= bar_o
    if N > 1:
        assert norms[2] == 0.0 and (out[2] == 0.0).all()
    # the package's helper is the same two launches
    hn, ho = _row_norms(_dev(x), EPS, normalize=True)
    assert np.array_equal(_bits(hn.cpu().numpy()), _bits(norms))
    assert np.array_equal(_bits(ho.cpu().numpy()), _bits(out))


@pytest.mark.parametrize("D", [1, 65, 257])
def test_zero_row_alone(D):
    norms, out = _row_norms_raw(np.zeros((1, D), dtype=np.float32))
    print(f"D={D}: zero row -> norm {norms[0]}, max |out| {np.abs(out).max()}")
    assert norms[0] == 0.0 and (out == 0.0).all()


# ------------------------------------------------------------------ b. class_sums / centroids
def _centroids_raw(x, labels, K, eps=EPS):
    """(sums [K, D], centroids [K, D]) of miclip_class_centroids, the CSR built as
    miclip.outliers._class_centroids builds it."""
    from miclip import _lib
    lib = _lib.load_library()
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=K))]).astype(np.int32)
    D = x.shape[1]
    xd, od, fd = _dev(x), _dev(order), _dev(offsets)
    sums, cent = _padded(K * D), _padded(K * D)
    _lib.check(lib.miclip_class_centroids(_ptr(xd), _ptr(od), _ptr(fd), K, D, eps, _ptr(sums),
                                          _ptr(cent), _lib.stream_handle()),
               "miclip_class_centroids")
    return _take(sums, K * D).reshape(K, D), _take(cent, K * D).reshape(K, D)


SIZES = (1, 7, 8, 9, 16, 17)            # on both sides of the unroll of 8


def _interleaved_labels(sizes, seed):
    lab = np.concatenate([np.full(n, k) for k, n in enumerate(sizes)])
    np.random.default_rng(seed).shuffle(lab)
    # really interleaved: no class is one contiguous run (but the singletons)
    for k, n in enumerate(sizes):
        idx = np.flatnonzero(lab == k)
        assert n < 7 or idx[-1] - idx[0] >= n
    return lab.astype(np.int64)


@pytest.mark.parametrize("D", [1, 63, 65, 130])
def test_class_sums_bit_exact_and_centroids(D):
    from miclip.outliers import _class_centroids
    lab = _interleaved_labels(SIZES, D)
    rng = np.random.default_rng(D)
    x = rng.standard_normal((len(lab), D)).astype(np.float32)
    K = len(SIZES)
    sums, cent = _centroids_raw(x, lab, K)
    want = R.class_sums_f32(x, lab, K)
    n_bad = int((_bits(sums) != _bits(want)).sum())
    err = float(np.abs(cent - R.centroids(x, lab, K)).max())
    bar = _bar(MEASURED_CENT, TOL_VEC)
    print(f"D={D}: sums differing in bits {n_bad} of {sums.size}; centroid err {err:.3g} (bar {bar:.3g})")
    assert np.array_equal(_bits(sums), _bits(want))
    assert err <= bar <= TOL_VEC
    hc, counts = _class_centroids(_dev(x), lab, K, EPS)
    assert np.array_equal(counts, np.asarray(SIZES))
    assert np.array_equal(_bits(hc.cpu().numpy()), _bits(cent))


@pytest.mark.parametrize("D,N", [(1, 1), (65, 19), (130, 8)])
def test_class_sums_single_class(D, N):
    x = np.random.default_rng(N).standard_normal((N, D)).astype(np.float32)
    lab = np.zeros(N, dtype=np.int64)
    sums, cent = _centroids_raw(x, lab, 1)
    err = float(np.abs(cent - R.centroids(x, lab, 1)).max())
    print(f"K=1 D={D} N={N}: centroid err {err:.3g} (bar {_bar(MEASURED_CENT, TOL_VEC):.3g})")
    assert np.array_equal(_bits(sums), _bits(R.class_sums_f32(x, lab, 1)))
    assert err <= _bar(MEASURED_CENT, TOL_VEC)


@pytest.mark.parametrize("D", [63, 130])
def test_empty_class_rows_are_zero_and_change_nothing(D):
    """An empty class: its sums row and its centroid row are exact zeros (kernels.h), and
    every other class's rows are those of the run without it, bit for bit."""
    from miclip.outliers import _class_centroids
    lab = _interleaved_labels(SIZES, 7 + D)
    x = np.random.default_rng(D).standard_normal((len(lab), D)).astype(np.float32)
    K = len(SIZES)
    sums, cent = _centroids_raw(x, lab, K)
    for empty in (0, 3, K):                 # first, middle, last
        lab2 = lab + (lab >= empty)
        s2, c2 = _centroids_raw(x, lab2, K + 1)
        keep = np.arange(K + 1) != empty
        print(f"D={D} empty class {empty}: sums row max |v| {np.abs(s2[empty]).max()}, centroid "
              f"row max |v| {np.abs(c2[empty]).max()}")
        assert (_bits(s2[empty]) == 0).all() and (_bits(c2[empty]) == 0).all()
        assert np.array_equal(_bits(s2[keep]), _bits(sums))
        assert np.array_equal(_bits(c2[keep]), _bits(cent))
        hc, counts = _class_centroids(_dev(x), lab2, K + 1, EPS)
        assert counts[empty] == 0 and np.array_equal(_bits(hc.cpu().numpy()), _bits(c2))


# ------------------------------------------------------------------ c. proto_scores
def _scores_raw(x, protos, owner, cls, inv_nx=None, inv_np=None):
    """(own_best, own_arg, other_best) of miclip_proto_scores on device tensors."""
    from miclip import _lib
    lib = _lib.load_library()
    N, D = x.shape
    P = protos.shape[0]
    own, arg, oth = _padded(N), _padded(N, torch.int32), _padded(N)
    _lib.check(lib.miclip_proto_scores(_ptr(x), _ptr(protos), _ptr(owner), _ptr(cls),
                                       _ptr(inv_nx), _ptr(inv_np), N, P, D, _ptr(own), _ptr(arg),
                                       _ptr(oth), _lib.stream_handle()), "miclip_proto_scores")
    return _take(own, N), _take(arg, N), _take(oth, N)


def _kernel_sim(x, protos):
    """The kernel's own sim [N, P]: the call with protos[p:p+1], owner = [0], cls = 0
    returns sim[:, p] as own_best (one tiny launch per prototype)."""
    from miclip import _lib
    lib = _lib.load_library()
    N, D = x.shape
    P = protos.shape[0]
    zero1 = torch.zeros(1, device="cuda", dtype=torch.int32)
    zeros = torch.zeros(N, device="cuda", dtype=torch.int32)
    cols = torch.full((P, N), CANARY_F, device="cuda")
    arg, oth = _padded(N, torch.int32), _padded(N)
    for p in range(P):
        _lib.check(lib.miclip_proto_scores(_ptr(x), _ptr(protos[p:p + 1]), _ptr(zero1), _ptr(zeros),
                                           None, None, N, 1, D, _ptr(cols[p]), _ptr(arg), _ptr(oth),
                                           _lib.stream_handle()), "miclip_proto_scores")
    assert (_take(arg, N) == 0).all() and (_take(oth, N) == -np.inf).all()
    return cols.cpu().numpy().T.copy()


def _unit(rng, n, d):
    a = rng.standard_normal((n, d))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def test_similarity_is_independent_of_the_tile_position():
    """The same prototype at index 0 (tile 0) and at index 64 (tile 1, P = 65), and alone:
    its column of similarities is the same bits."""
    rng = np.random.default_rng(65)
    N, P, D = 130, 65, 17
    x, pr = _unit(rng, N, D), _unit(rng, P, D)
    pr[64] = pr[0]
    xd, pd = _dev(x), _dev(pr)
    cls = torch.zeros(N, device="cuda", dtype=torch.int32)
    cols = []
    for p in (0, 64):
        owner = np.ones(P, dtype=np.int32)
        owner[p] = 0
        own, arg, _ = _scores_raw(xd, pd, _dev(owner), cls)
        assert (arg == p).all()
        cols.append(own)
    alone = _kernel_sim(xd, pd[:1])[:, 0]
    n1 = int((_bits(cols[0]) != _bits(cols[1])).sum())
    n2 = int((_bits(cols[0]) != _bits(alone)).sum())
    print(f"similarities differing in bits: index 0 vs 64: {n1}, vs the single-prototype call: {n2}")
    assert n1 == 0 and n2 == 0


# every N of {1, 63, 65, 130}, P of {1, 5, 64, 65, 129}, D of {1, 3, 15, 17, 96}
PROTO_SHAPES = [(1, 1, 1), (1, 129, 17), (63, 5, 3), (63, 64, 96), (65, 1, 15), (65, 65, 17),
                (65, 129, 3), (130, 5, 96), (130, 64, 1), (130, 65, 15), (130, 129, 96),
                (63, 65, 1)]


def _proto_case(N, P, D, seed):
    """Unit-norm x and prototypes, K = 4 classes; duplicated prototype rows of one class
    at (p, p + 1), (p, p + 4) and (p, p + 64) where P allows, and samples aimed at them
    so that the duplicates are their best own prototype; class 3 owns no prototype."""
    rng = np.random.default_rng(seed)
    x = _unit(rng, N, D)
    pr = _unit(rng, P, D)
    owner = rng.integers(0, 3, P).astype(np.int32)
    cls = rng.integers(0, 4, N).astype(np.int32)       # class 3: no own prototype
    dups = [(a, b) for a, b in ((1, 2), (0, 4), (3, 3 + 64)) if b < P]
    for i, (a, b) in enumerate(dups):
        pr[b] = pr[a]
        owner[a] = owner[b] = i % 3
        for s in range(i, N, 5):                       # samples aimed at the pair
            x[s], cls[s] = pr[a], owner[a]
    return x, pr, owner, cls, dups


@pytest.mark.parametrize("N,P,D", PROTO_SHAPES)
def test_proto_scores_exact_on_own_similarities(N, P, D):
    x, pr, owner, cls, dups = _proto_case(N, P, D, 1000 * N + 10 * P + D)
    xd, pd = _dev(x), _dev(pr)
    sim = _kernel_sim(xd, pd)
    for a, b in dups:           # the precondition: duplicated rows tie bit for bit
        assert np.array_equal(_bits(sim[:, a]), _bits(sim[:, b]))
    ref = x.astype(np.float64) @ pr.astype(np.float64).T
    err = float(np.abs(sim - ref).max())
    bar = _bar(MEASURED_SIM, TOL_SIM)
    own, arg, oth = _scores_raw(xd, pd, _dev(owner), _dev(cls))
    w_own, w_arg, w_oth = R.proto_reduce(sim, owner, cls)
    tied = int(sum((sim[s, owner == cls[s]] == w_own[s]).sum() > 1 for s in range(N)))
    print(f"N={N} P={P} D={D}: sim err {err:.3g} (bar {bar:.3g}); rows with an exact own-class "
          f"tie {tied}, without own prototype {int((w_arg < 0).sum())}; mismatches own "
          f"{int((_bits(own) != _bits(w_own)).sum())} arg {int((arg != w_arg).sum())} other "
          f"{int((_bits(oth) != _bits(w_oth)).sum())}")
    assert err <= bar <= TOL_SIM
    if dups and N >= 5:
        assert tied > 0
    assert np.array_equal(_bits(own), _bits(w_own))
    assert np.array_equal(arg, w_arg)
    assert np.array_equal(_bits(oth), _bits(w_oth))
    none = cls == 3
    assert (own[none] == -np.inf).all() and (arg[none] == -1).all()


@pytest.mark.parametrize("N,P,D", [(1, 1, 3), (65, 5, 17), (130, 65, 15)])
def test_proto_scores_no_own_and_no_other_prototype(N, P, D):
    """With inv_nx / inv_np given: a class that owns no prototype gives -inf / -1, a call
    where every prototype is the sample's own gives other_best = -inf."""
    rng = np.random.default_rng(N + P + D)
    x, pr = _unit(rng, N, D) * 3.0, _unit(rng, P, D) * 0.5
    xd, pd = _dev(x), _dev(pr)
    inx = _dev(np.full(N, 1 / 3.0, dtype=np.float32))
    inp = _dev(np.full(P, 2.0, dtype=np.float32))
    zeros_p = torch.zeros(P, device="cuda", dtype=torch.int32)
    cls = np.zeros(N, dtype=np.int32)
    cls[::2] = 1                                        # class 1 owns nothing
    own, arg, oth = _scores_raw(xd, pd, zeros_p, _dev(cls), inx, inp)
    ref = (x.astype(np.float64) @ pr.astype(np.float64).T) * (np.float32(1 / 3.0) * 2.0)
    mine = cls == 0
    print(f"N={N} P={P} D={D}: rows without own prototype {int((~mine).sum())}, without other "
          f"{int(mine.sum())}")
    assert (own[~mine] == -np.inf).all() and (arg[~mine] == -1).all()
    assert (oth[mine] == -np.inf).all()
    bar = _bar(MEASURED_COS, TOL_SIM)
    if mine.any():
        e = float(np.abs(own[mine] - ref[mine].max(axis=1)).max())
        print(f"  own_best err {e:.3g} (bar {bar:.3g})")
        assert e <= bar and ((arg[mine] >= 0) & (arg[mine] < P)).all()
    e = float(np.abs(oth[~mine] - ref[~mine].max(axis=1)).max())
    print(f"  other_best err {e:.3g} (bar {bar:.3g})")
    assert e <= bar <= TOL_SIM


@pytest.mark.parametrize("N,P,D", [(63, 5, 3), (65, 65, 17), (130, 129, 96)])
def test_proto_scores_inverse_norms_against_fp64(N, P, D):
    """The cosine with inv_nx / inv_np given, and the null call on pre-scaled inputs:
    both against float64 (the two round differently, so not bit equality)."""
    rng = np.random.default_rng(3 * N + P + D)
    x = _unit(rng, N, D) * np.exp(rng.uniform(-2, 2, (N, 1))).astype(np.float32)
    pr = _unit(rng, P, D) * np.exp(rng.uniform(-2, 2, (P, 1))).astype(np.float32)
    owner = rng.integers(0, 3, P).astype(np.int32)
    cls = rng.integers(0, 3, N).astype(np.int32)
    inx = (1.0 / np.maximum(R.row_norms(x), EPS)).astype(np.float32)
    inp = (1.0 / np.maximum(R.row_norms(pr), EPS)).astype(np.float32)
    cos = (x.astype(np.float64) @ pr.astype(np.float64).T) * inx[:, None].astype(np.float64) \
        * inp[None].astype(np.float64)
    xs, ps = (x * inx[:, None]).astype(np.float32), (pr * inp[:, None]).astype(np.float32)
    cos_s = xs.astype(np.float64) @ ps.astype(np.float64).T
    bar = _bar(MEASURED_COS, TOL_SIM)
    worst = 0.0
    for tag, args, ref in (("inverse norms", (_dev(x), _dev(pr), _dev(owner), _dev(cls), _dev(inx),
                                              _dev(inp)), cos),
                           ("pre-scaled", (_dev(xs), _dev(ps), _dev(owner), _dev(cls)), cos_s)):
        own, arg, oth = _scores_raw(*args)
        same = cls[:, None] == owner[None]
        w_own = np.where(same, ref, -np.inf).max(axis=1)
        w_oth = np.where(~same, ref, -np.inf).max(axis=1)
        has, hoth = np.isfinite(w_own), np.isfinite(w_oth)
        e = max(float(np.abs(own[has] - w_own[has]).max()) if has.any() else 0.0,
                float(np.abs(oth[hoth] - w_oth[hoth]).max()) if hoth.any() else 0.0)
        worst = max(worst, e)
        print(f"N={N} P={P} D={D} {tag}: best-value err {e:.3g} (bar {bar:.3g})")
        assert (own[~has] == -np.inf).all() and (arg[~has] == -1).all()
        assert (oth[~hoth] == -np.inf).all()
        # the chosen prototype is an own one whose fp64 cosine is within the bar of the best
        pick = ref[np.arange(N)[has], arg[has]]
        assert same[np.arange(N)[has], arg[has]].all() and (w_own[has] - pick <= 2 * bar).all()
    assert worst <= bar <= TOL_SIM
