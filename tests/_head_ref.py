"""fp64 numpy restatement of the kernels that turn features into what a user reads,
CPU only: the yardstick of tests/test_gpu_head_edges.py and
tests/test_gpu_scoring_edges.py. It touches nothing under test.

  head      scale * normalize(f [@ proj]) @ tw, top-k, token embed + EOT + ln_final
            (csrc/embed.hip: head_proj_kernel, head_logits_kernel, topk_rows_kernel,
            token_embed_kernel, eot_kernel)
  scoring   row norms, per-class sums / centroids, prototype scores (csrc/scoring.hip)

The self-checks at the bottom (tests/test_host_logic.py style, run by the CPU part of
tests/test_gpu_head_edges.py) compare these functions with torch in float64.
"""
import numpy as np

U24 = 2.0 ** -24        # fp32 unit roundoff
EPS = 1e-12             # F.normalize's eps


# ------------------------------------------------------------------ head
def logits(f, tw, scale, proj=None):
    """scale * (p / max(|p|, 1e-12)) @ tw with p = f @ proj (or f), float64 throughout
    on the given (fp32) inputs."""
    p = np.asarray(f, dtype=np.float64)
    if proj is not None:
        p = p @ np.asarray(proj, dtype=np.float64)
    n = np.maximum(np.sqrt((p * p).sum(axis=1, keepdims=True)), EPS)
    return scale * ((p / n) @ np.asarray(tw, dtype=np.float64))


def logits_cap(scale, E, Din=0):
    """Worst-case absolute error of an fp32 logit for unit-norm text columns: E exact-
    product fp32 accumulations (E * 2^-24 of sum |f_d tw_dc| <= 1 by Cauchy-Schwarz) and
    8 more roundings for the norm, the reciprocal and the two scalings; with the
    projection its Din accumulations come on top."""
    return scale * (E + Din + 8) * U24


def topk(z, k):
    """torch.topk(sorted=True)'s order by a lexsort: NaN above every number, then value
    descending, the lower index first among NaNs and among equal values."""
    z = np.asarray(z)
    nan = np.isnan(z)
    neg = np.where(nan, 0.0, -z.astype(np.float64))
    idx = np.broadcast_to(np.arange(z.shape[1]), z.shape)
    out = np.empty((z.shape[0], k), dtype=np.int32)
    for r in range(z.shape[0]):         # keys: last = primary
        out[r] = np.lexsort((idx[r], neg[r], ~nan[r]))[:k]
    return out


def first_argmax(tokens):
    """torch.argmax(-1): the first position of each row's maximum."""
    tokens = np.asarray(tokens)
    return np.array([int(np.flatnonzero(row == row.max())[0]) for row in tokens], dtype=np.int64)


def layernorm(x, gamma, beta, eps=1e-5):
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def text_eot_features(tokens, tok_emb, pos, gamma, beta, resid16):
    """encode_text's x_before with no transformer block: LN_1e-5(r(tok_emb[id] + pos[t*])),
    t* = the first arg-max of the prompt; the sum is one fp32 add, r rounds it to fp16
    (the fp16 residual stream) or is the identity."""
    tokens = np.asarray(tokens)
    t = first_argmax(tokens)
    ids = tokens[np.arange(len(t)), t]
    x = np.asarray(tok_emb, np.float32)[ids] + np.asarray(pos, np.float32)[t]
    if resid16:
        x = x.astype(np.float16)
    return layernorm(x.astype(np.float64), gamma, beta), t


# ------------------------------------------------------------------ scoring
def row_norms(x):
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt((x * x).sum(axis=1))


def div_rows(x, eps=EPS):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(row_norms(x), eps)[:, None]


def class_sums_f32(x, labels, K):
    """Strict sequential fp32 accumulation in ascending sample order (what a CPU
    index_add_ does): sums[labels[i]] += x[i] for i = 0, 1, ..."""
    x = np.asarray(x, dtype=np.float32)
    sums = np.zeros((K, x.shape[1]), dtype=np.float32)
    for i, k in enumerate(np.asarray(labels)):
        sums[k] = sums[k] + x[i]
    return sums


def centroids(x, labels, K, eps=EPS):
    """normalize(per-class mean) in fp64; an empty class gives a zero row."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((K, x.shape[1]))
    for k in range(K):
        rows = x[np.asarray(labels) == k]
        if len(rows):
            m = rows.mean(axis=0)
            out[k] = m / max(np.sqrt((m * m).sum()), eps)
    return out


def proto_reduce(sim, owner, cls):
    """(own_best, own_arg, other_best) of a similarity matrix [N, P]: the maximum and its
    FIRST index over the prototypes of the sample's class (-inf / -1 when it owns none),
    the maximum over the others (-inf when there are none). Values are taken from sim
    as they are (no arithmetic), so on the kernel's own fp32 sim the result is exact."""
    sim, owner, cls = np.asarray(sim), np.asarray(owner), np.asarray(cls)
    n = sim.shape[0]
    own = np.full(n, -np.inf, dtype=sim.dtype)
    arg = np.full(n, -1, dtype=np.int32)
    oth = np.full(n, -np.inf, dtype=sim.dtype)
    for s in range(n):
        mine = owner == cls[s]
        if mine.any():
            idx = np.flatnonzero(mine)
            j = idx[int(np.argmax(sim[s, idx]))]    # np.argmax: the first maximum
            own[s], arg[s] = sim[s, j], j
        if (~mine).any():
            oth[s] = sim[s, ~mine].max()
    return own, arg, oth


# ------------------------------------------------------------------ self-checks (CPU)
def selfcheck_topk():
    import torch
    rng = np.random.default_rng(0)
    z = rng.standard_normal((40, 23)).astype(np.float32)
    for k in (1, 3, 23):
        want = torch.topk(torch.from_numpy(z).double(), k, dim=1).indices.numpy()
        assert np.array_equal(topk(z, k), want)
    # ties, infinities and NaN: the documented order, and torch.topk's VALUES (its
    # indices among equals / NaNs are not specified, the values are)
    z = np.array([[1.0, 3.0, 3.0, np.nan, -np.inf, np.inf, np.nan, 3.0],
                  [np.nan] * 8,
                  [2.0] * 8,
                  [0.0, -0.0, np.inf, np.inf, -np.inf, -np.inf, 0.0, 5.0]], dtype=np.float32)
    got = topk(z, 8)
    assert got[0].tolist() == [3, 6, 5, 1, 2, 7, 0, 4]
    assert got[1].tolist() == list(range(8)) and got[2].tolist() == list(range(8))
    assert got[3].tolist() == [2, 3, 7, 0, 1, 6, 4, 5]
    tv = torch.topk(torch.from_numpy(z).double(), 8, dim=1).values.numpy()
    mine = np.take_along_axis(z.astype(np.float64), got.astype(np.int64), axis=1)
    assert np.array_equal(np.isnan(mine), np.isnan(tv))
    assert np.array_equal(np.nan_to_num(mine, nan=7.0), np.nan_to_num(tv, nan=7.0))
    for k in (1, 3):
        assert np.array_equal(topk(z, k), got[:, :k])


def selfcheck_text():
    import torch
    rng = np.random.default_rng(1)
    tok = rng.integers(0, 9, (50, 70))
    tok[0] = 8                      # every position equal
    tok[1, [5, 69]] = 30            # a repeated maximum
    tok[2, 69] = 31                 # the maximum last
    want = torch.argmax(torch.from_numpy(tok), dim=-1).numpy()
    assert np.array_equal(first_argmax(tok), want) and want[0] == 0 and want[1] == 5
    W = 32
    emb = rng.standard_normal((40, W)).astype(np.float32)
    pos = rng.standard_normal((70, W)).astype(np.float32)
    gam = (1 + 0.1 * rng.standard_normal(W)).astype(np.float32)
    bet = (0.05 * rng.standard_normal(W)).astype(np.float32)
    for r16 in (False, True):
        got, t = text_eot_features(tok, emb, pos, gam, bet, r16)
        x = torch.from_numpy(emb)[torch.from_numpy(tok)] + torch.from_numpy(pos)[None]
        x = x[torch.arange(50), torch.from_numpy(want)]
        if r16:
            x = x.half()
        ref = torch.nn.functional.layer_norm(x.double(), (W,), torch.from_numpy(gam).double(),
                                             torch.from_numpy(bet).double(), 1e-5).numpy()
        assert np.abs(got - ref).max() <= 1e-12 and np.array_equal(t, want)


def selfcheck_head_and_scoring():
    import torch
    rng = np.random.default_rng(2)
    f = rng.standard_normal((7, 32)).astype(np.float32)
    f[3] = 0.0
    proj = rng.standard_normal((32, 16)).astype(np.float32)
    tw = rng.standard_normal((16, 5)).astype(np.float32)
    tf, tp, tt = (torch.from_numpy(a).double() for a in (f, proj, tw))
    ref = 100.0 * torch.nn.functional.normalize(tf @ tp, dim=-1) @ tt
    assert np.abs(logits(f, tw, 100.0, proj) - ref.numpy()).max() <= 1e-11
    assert (logits(f, tw, 100.0, proj)[3] == 0).all()
    assert np.abs(div_rows(f) - torch.nn.functional.normalize(tf, dim=-1).numpy()).max() <= 1e-15
    lab = rng.integers(0, 4, 7)
    lab[lab == 2] = 3               # class 2 empty
    sums = torch.zeros(4, 32).index_add_(0, torch.from_numpy(lab), torch.from_numpy(f))
    assert np.array_equal(class_sums_f32(f, lab, 4), sums.numpy())
    c = centroids(f, lab, 4)
    assert (c[2] == 0).all() and abs(np.linalg.norm(c[3]) - 1) <= 1e-12
    sim = rng.standard_normal((6, 5)).astype(np.float32)
    sim[:, 3] = sim[:, 1]           # an exact tie inside class 0
    owner, cls = np.array([0, 0, 1, 0, 1]), np.array([0, 0, 1, 2, 0, 1])
    own, arg, oth = proto_reduce(sim, owner, cls)
    ts = torch.from_numpy(sim)
    same = torch.from_numpy(cls)[:, None] == torch.from_numpy(owner)[None]
    m = ts.masked_fill(~same, -np.inf).max(1)
    assert np.array_equal(own, m.values.numpy()) and own[3] == -np.inf and arg[3] == -1
    assert np.array_equal(oth, ts.masked_fill(same, -np.inf).max(1).values.numpy())
    for s in (0, 1, 4):             # the first index of the maximum
        assert arg[s] == min(j for j in (0, 1, 3) if sim[s, j] == own[s])
