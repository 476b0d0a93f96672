"""fp64 numpy restatement of the fused multi-head attention over a packed QKV buffer
(csrc/attention.hip), CPU only: the yardstick of tests/test_gpu_attention_edges.py,
checked against torch in float64 by tests/test_attn_ref.py. It touches nothing under test.

Layout: qkv [B*N, 3*H*dh], columns q | k | v, each [H, dh]; out [B*N, H*dh].

  attention             softmax(q k^T / sqrt(dh) [+ causal mask]) v in float64 on the given
                        (already rounded) operands, and the error unit
                        U[q, d] = sum_k p[q, k] |v[k, d]|
  reference_arithmetic  the same with the roundings the reference model's torch path performs
                        on dtype-T tensors: q / sqrt(dh), the scores, the softmax output and
                        P V are rounded to T, every product itself is float64
  bar                   the per-element bound max(4, E_T) u U, E_T the reference arithmetic's
                        own error in units of u U
  random / indicator_v / one_hot / staircase
                        the input families, deterministic from a seed, rounded to T
"""
import numpy as np

UNIT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}     # unit roundoff of the compute dtype
LOG2E = 1.4426950408889634


# ------------------------------------------------------------------ rounding to T
def round_to(x, T):
    """x -> float32 -> T (round to nearest even, what a cast of an fp32 result does),
    returned as float64."""
    x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    if T == "fp16":
        return x32.astype(np.float16).astype(np.float64)
    assert T == "bf16", T
    bits = x32.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def is_exact(x, T):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.array_equal(round_to(x, T), x))


# ------------------------------------------------------------------ layout
def split(qkv, B, N, H, dh):
    """(q, k, v), each [B, H, N, dh] float64."""
    x = np.asarray(qkv, dtype=np.float64).reshape(B, N, 3, H, dh)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))


def pack(q, k, v):
    """[B, H, N, dh] x 3 -> qkv [B*N, 3*H*dh]."""
    B, H, N, dh = q.shape
    x = np.stack([a.transpose(0, 2, 1, 3) for a in (q, k, v)], axis=2)      # [B, N, 3, H, dh]
    return np.ascontiguousarray(x.reshape(B * N, 3 * H * dh))


def merge(o):
    """[B, H, N, dh] -> [B*N, H*dh]."""
    B, H, N, dh = o.shape
    return np.ascontiguousarray(o.transpose(0, 2, 1, 3).reshape(B * N, H * dh))


def visible(N, causal):
    """[N, N] bool: key k (column) is attended to by query q (row)."""
    if not causal:
        return np.ones((N, N), dtype=bool)
    return np.tril(np.ones((N, N), dtype=bool))


# ------------------------------------------------------------------ the yardstick
def attend(q, k, v, causal):
    """(out, U) of stacks [..., N, dh] in float64."""
    N, dh = q.shape[-2:]
    s = (q @ np.swapaxes(k, -1, -2)) * dh ** -0.5
    s = np.where(visible(N, causal), s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    return p @ v, p @ np.abs(v)


def attention(qkv, B, N, H, dh, causal):
    """(out [B*N, H*dh], U [B*N, H*dh]) in float64 on the operands as given."""
    q, k, v = split(qkv, B, N, H, dh)
    o, U = attend(q, k, v, causal)
    return merge(o), merge(U)


def reference_arithmetic(qkv, B, N, H, dh, causal, T):
    """out [B*N, H*dh] with the roundings of nn.MultiheadAttention's math path on dtype-T
    tensors: r(q * dh^-1/2), r(q' k^T) (+ the -inf mask), r(softmax in fp32), r(P V)."""
    q, k, v = split(qkv, B, N, H, dh)
    qs = round_to(q * dh ** -0.5, T)
    s = round_to(qs @ np.swapaxes(k, -1, -2), T)
    s = np.where(visible(N, causal), s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p = round_to(p / p.sum(axis=-1, keepdims=True), T)
    return merge(round_to(p @ v, T))


def ratio(got, out, U, u):
    """Largest |got - out| / (u U); an element with U = 0 counts 0 if exact, inf if not."""
    err = np.abs(np.asarray(got, dtype=np.float64) - out)
    pos = U > 0
    r = float((err[pos] / (u * U[pos])).max()) if pos.any() else 0.0
    if (err[~pos] != 0).any():
        r = float("inf")
    return r


def e_t(out, U, ref_T, u):
    """E_T: the reference arithmetic's own error, max over the elements with U > 0 of
    |ref_T - out| / (u U)."""
    pos = U > 0
    return float((np.abs(ref_T - out)[pos] / (u * U[pos])).max()) if pos.any() else 0.0


def bar(out, U, ref_T, u):
    """The per-element bound max(4, E_T) u U (0 where U = 0: those must be exact).
    4: P rounded to T, a differently rounded P in the row sum, the rounded output (each
    <= u U to first order), and one unit for fp32 accumulation and v_exp_f32."""
    return max(4.0, e_t(out, U, ref_T, u)) * u * U


def within(got, out, bound):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - out) <= bound).all())


# ------------------------------------------------------------------ input families
def random(B, N, H, dh, T, seed):
    """N(0, 1.5^2), the inputs of tests/test_gpu_kernels.py."""
    rng = np.random.default_rng(seed)
    return round_to(1.5 * rng.standard_normal((B * N, 3 * H * dh)), T)


def indicator_keys(N):
    """The keys an indicator-V head may single out, most telling first: the last key, the
    256-key pass boundary of the CLS kernel, the first key of the last 32-key tile, the
    first key, the one before last, the 32-key tile boundary."""
    cand = [N - 1, 256, 255, 32 * ((N - 1) // 32), 0, N - 2, 32, 31]
    keys = []
    for c in cand:
        if 0 <= c < N and c not in keys:
            keys.append(c)
    return keys


def indicator_v(B, N, H, dh, T, seed, causal):
    """q = 0 (a flat softmax), K random, V zero except row k* of each head, V[k*, d] =
    (d + 1) / 8. Returns (qkv, kstar [B, H], expected out [B*N, H*dh]): the expected
    output is V[k*] [k* visible] / count(q), count = N, or q + 1 when causal."""
    rng = np.random.default_rng(seed)
    k = round_to(1.5 * rng.standard_normal((B, H, N, dh)), T)
    q = np.zeros_like(k)
    v = np.zeros_like(k)
    keys = indicator_keys(N)
    kstar = np.zeros((B, H), dtype=np.int64)
    row = (np.arange(dh) + 1) / 8.0
    want = np.zeros_like(k)
    qi = np.arange(N)
    for b in range(B):
        for h in range(H):
            ks = keys[(b * H + h) % len(keys)]
            kstar[b, h] = ks
            v[b, h, ks] = row
            if causal:
                want[b, h] = np.where(qi >= ks, 1.0 / (qi + 1), 0.0)[:, None] * row
            else:
                want[b, h] = row / N
    return pack(q, k, v), kstar, merge(want)


def one_hot_target(N, causal):
    i = np.arange(N)
    return np.where(causal, (37 * i + 5) % (i + 1), (37 * i + 5) % N)


def one_hot(B, N, H, dh, T, seed, causal):
    """K entries +-4 at random, q_i = K[t(i)], t(i) = (37 i + 5) mod N (mod i + 1 when
    causal), V random. Returns (qkv, t [N], expected out = V[t(i)])."""
    rng = np.random.default_rng(seed)
    k = 4.0 * rng.choice([-1.0, 1.0], size=(B, H, N, dh))
    v = round_to(1.5 * rng.standard_normal((B, H, N, dh)), T)
    t = one_hot_target(N, causal)
    return pack(k[:, :, t], k, v), t, merge(v[:, :, t])


def one_hot_margin(qkv, B, N, H, dh, causal):
    """The smallest gap, in log2 units of the softmax, between the score of the target key
    and of any other visible key (inf where the target is the only one)."""
    q, k, _ = split(qkv, B, N, H, dh)
    s = (q @ np.swapaxes(k, -1, -2)) * (dh ** -0.5 * LOG2E)
    t = one_hot_target(N, causal)
    top = s[..., np.arange(N), t]
    other = np.where(visible(N, causal), s, -np.inf)
    other[..., np.arange(N), t] = -np.inf
    return float((top - other.max(axis=-1)).min())


STEPS = (12.0, -12.0, 7.5, 8.5)     # log2 units per 32-key tile; 8 is the lazy-rescale threshold


def staircase(B, N, H, dh, T, seed, step):
    """N(0, 1) with q[:, 0] = 8 and K[j, 0] = floor(j / 32) step / (8 c2), c2 = log2(e) /
    sqrt(dh): dim 0 lifts the log2-domain score of every query by `step` per 32-key tile
    (up to the rounding of K[j, 0] to T)."""
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((B, H, N, dh)) for _ in range(3))
    c2 = LOG2E * dh ** -0.5
    q[..., 0] = 8.0
    k[..., 0] = (np.arange(N) // 32) * step / (8.0 * c2)
    return round_to(pack(q, k, v), T)


def staircase_steps(qkv, B, N, H, dh):
    """Per tile boundary, the rise of dim 0's log2-domain score contribution [ntiles - 1]
    (identical for every head and query by construction)."""
    q, k, _ = split(qkv, B, N, H, dh)
    c2 = LOG2E * dh ** -0.5
    lift = q[0, 0, 0, 0] * k[0, 0, ::32, 0] * c2
    return np.diff(lift)
