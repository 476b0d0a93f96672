"""CPU: the float64 yardstick of the device k-means (tests/_kmeans_ref.py) against
scikit-learn's own Lloyd loop, KMeans(init=C0, n_init=1, algorithm="lloyd") on fp32
data. Each shape runs from random-row initial centres and once from a planted far
centre that empties a cluster in the first iteration (the relocation rule).

Bars: labels and n_iter_ equal; centres within 1e-6 absolute and inertia within 1e-6
relative. scikit-learn fits fp32 data in fp32, which is what those two bars hold
(7.6e-8 and 1.6e-7 were measured); a wrong rule shows at 1e-2.
"""
import warnings

import numpy as np
import pytest

import _kmeans_ref as K

SHAPES = [(2, 1, 2, 100), (33, 17, 3, 100), (240, 96, 4, 100), (240, 96, 4, 2),
          (600, 130, 6, 100), (64, 768, 4, 100)]


def _case(n, D, k, init, seed=0):
    x, _ = K.planted(n, D, k, seed=100 + seed)
    if D == 1:     # k directions in one dimension are only +-1: spread the rows instead
        x = np.random.default_rng(7 + seed).standard_normal((n, 1)).astype(np.float32)
    rng = np.random.default_rng(1000 + seed)
    c0 = x[rng.choice(n, k, replace=False)].astype(np.float64)
    if init == "empty":
        c0[k - 1] = 10.0 * np.sign(c0[k - 1].sum() + 0.5)     # far from every row
    return x, c0


@pytest.mark.parametrize("init", ["rows", "empty"])
@pytest.mark.parametrize("n,D,k,max_iter", SHAPES)
def test_yardstick_lloyd_equals_sklearn(n, D, k, max_iter, init):
    from sklearn import cluster
    x, c0 = _case(n, D, k, init)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = cluster.KMeans(n_clusters=k, init=c0.astype(np.float32), n_init=1, max_iter=max_iter,
                            algorithm="lloyd", tol=1e-4).fit(x)
    fit = K.lloyd(x, c0.astype(np.float32), max_iter, K.tol_of(x))
    if init == "empty":
        assert fit.relocated >= 1, "the planted centre did not empty a cluster"
    assert np.array_equal(fit.labels, km.labels_)
    assert fit.n_iter == km.n_iter_
    dc = float(np.abs(fit.centres - km.cluster_centers_.astype(np.float64)).max())
    di = abs(fit.inertia - float(km.inertia_)) / max(fit.inertia, 1e-300)
    print(f"n={n} D={D} k={k} max_iter={max_iter} {init}: centres {dc:.2e} inertia rel {di:.2e} "
          f"n_iter {fit.n_iter} strict {fit.strict} min gap {fit.min_gap:.2e}")
    assert dc <= 1e-6
    assert di <= 1e-6
