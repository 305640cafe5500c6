"""Float64 oracle of the three LoRA kernels (csrc/kernels/lora.hip) with an elementwise derived
error bound, and an op-by-op ``np.float32`` emulation.

numpy on the host, written from the definitions; it shares no code with the kernels or their torch
twins (``ddl25spring_amd.ops.lora``), both of which are checked against it.

The oracle takes the SAME fp32 operands as the code under test (``scale`` rounded to fp32) and
evaluates each product in float64. The bound is the classical one for a sum of n terms formed in
fp32 in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1):
with u = 2^-24 and gamma_n = n u / (1 - n u),

    |fl(sum_i a_i b_i) - sum_i a_i b_i| <= gamma_n sum_i |a_i b_i|,

whether the products are rounded on their own (plain fp32) or fused into the add (the fp32 MFMA is
an ``fmaf`` chain). Chained products multiply: (1 + gamma_a)(1 + gamma_b) <= 1 + gamma_(a + b). So

  fwd    u  = x A^T                  n = D
         y  = y0 + s (u B^T)         n = D + r + 4   (the two chains, the scale, the final add,
                                                      the four-wave fold of u) on |y0| + |s| |x||A|^T|B|^T
  bwd_x  v  = s (dy B)               n = N + 2
         dx = dx0 + v A              n = N + r + 4   on |dx0| + |s| |dy||B||A|
  bwd_w  dA = dA0 + v^T x            n = T + chunks + 3  on |dA0| + |v|^T|x|     (u, v are operands)
         dB = dB0 + s (dy^T u)       n = T + chunks + 3  on |dB0| + |s| |dy|^T|u|

``chunks = ceil(T / chunk)`` is the fold depth of the kernel's per-chunk partials. Nothing here is
fitted to any output: ``emulate_*`` shows that straightforward fp32 code meets the bound, and
tests/test_lora_cpu.py asserts that on every case before a kernel is judged by it.
"""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def _f64(t):
    return t.detach().cpu().double().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float64)


def _f32(t):
    return t.detach().cpu().float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def s32(x):
    return float(np.float32(x))


class Q:
    """value and absolute error bound of its fp32 counterpart."""

    def __init__(self, v, e):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)


def _t(a):
    return np.swapaxes(a, 1, 2)


def fwd(x, A, B, y0, scale):
    """x [S, T, D], A [S, r, D], B [S, N, r], y0 [S, T, N] -> (u, y) as Q."""
    x, A, B, y0, s = _f64(x), _f64(A), _f64(B), _f64(y0), s32(scale)
    D, r = A.shape[2], A.shape[1]
    u = x @ _t(A)
    mu = np.abs(x) @ _t(np.abs(A))
    y = y0 + s * (u @ _t(B))
    my = np.abs(y0) + abs(s) * (mu @ _t(np.abs(B)))
    return Q(u, gamma(D) * mu), Q(y, gamma(D + r + 4) * my)


def bwd_x(dy, A, B, dx0, scale):
    """-> (v, dx) as Q; dx0 None: dx = v A."""
    dy, A, B, s = _f64(dy), _f64(A), _f64(B), s32(scale)
    N, r = B.shape[1], B.shape[2]
    v = s * (dy @ B)
    mv = abs(s) * (np.abs(dy) @ np.abs(B))
    d0 = np.zeros(dy.shape[:2] + (A.shape[2],)) if dx0 is None else _f64(dx0)
    dx = d0 + v @ A
    mdx = np.abs(d0) + mv @ np.abs(A)
    return Q(v, gamma(N + 2) * mv), Q(dx, gamma(N + r + 4) * mdx)


def bwd_w(x, dy, u, v, dA0, dB0, scale, chunk):
    """u, v are operands (the fp32 tensors the kernel is given) -> (dA, dB) as Q."""
    x, dy, u, v, s = _f64(x), _f64(dy), _f64(u), _f64(v), s32(scale)
    T = x.shape[1]
    n = T + (T + chunk - 1) // chunk + 3
    dA0, dB0 = _f64(dA0), _f64(dB0)
    dA = dA0 + _t(v) @ x
    mA = np.abs(dA0) + _t(np.abs(v)) @ np.abs(x)
    dB = dB0 + s * (_t(dy) @ u)
    mB = np.abs(dB0) + abs(s) * (_t(np.abs(dy)) @ np.abs(u))
    return Q(dA, gamma(n) * mA), Q(dB, gamma(n) * mB)


# ------------------------------------------------------------------- plain fp32, one op at a time
def _dot32(a, b):
    """a [S, M, K] . b [S, K, N] in np.float32: products rounded, added in ascending k from 0."""
    S, M, Kd = a.shape
    acc = np.zeros((S, M, b.shape[2]), dtype=np.float32)
    for k in range(Kd):
        acc = acc + a[:, :, k:k + 1] * b[:, k:k + 1, :]
    assert acc.dtype == np.float32
    return acc


def emulate_fwd(x, A, B, y0, scale):
    x, A, B, y0, s = _f32(x), _f32(A), _f32(B), _f32(y0), np.float32(scale)
    u = _dot32(x, _t(A))
    y = y0 + s * _dot32(u, _t(B))
    return u, y


def emulate_bwd_x(dy, A, B, dx0, scale):
    dy, A, B, s = _f32(dy), _f32(A), _f32(B), np.float32(scale)
    v = s * _dot32(dy, B)
    p = _dot32(v, A)
    return v, (p if dx0 is None else _f32(dx0) + p)


def emulate_bwd_w(x, dy, u, v, dA0, dB0, scale, chunk):
    """Per-chunk partial sums, folded in chunk order, as the kernel does."""
    x, dy, u, v, s = _f32(x), _f32(dy), _f32(u), _f32(v), np.float32(scale)
    T = x.shape[1]
    pa = pb = None
    for t0 in range(0, T, chunk):
        sl = slice(t0, min(T, t0 + chunk))
        a, b = _dot32(_t(v[:, sl]), x[:, sl]), _dot32(_t(dy[:, sl]), u[:, sl])
        pa, pb = (a, b) if pa is None else (pa + a, pb + b)
    return _f32(dA0) + pa, _f32(dB0) + s * pb


def ratio(got, want: Q):
    """worst |got - value| / bound over the array (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(_f64(got) - want.v)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / want.e)
    return float(np.max(r)) if r.size else 0.0
