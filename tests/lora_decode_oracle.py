"""Float64 oracle of the per-sequence adapter kernels of the decode step (``ddl_lora_rows_u``,
``ddl_lin_rows_lora_f32`` in csrc/kernels/llama_decode.hip) with an elementwise derived error bound,
and the merged float64 twin of an adapted weight.

numpy on the host, written from the definitions; it shares no code with the kernels or their torch
twins (``ddl25spring_amd.ops.llama_decode``), both of which are checked against it.

The oracle takes the SAME fp32 operands as the code under test (``scale`` rounded to fp32) and
evaluates every expression in float64. The bound is Higham's (Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 3.1) for a sum of n terms formed in fp32 in any order, fused or not:
with u = 2^-24 and gamma_n = n u / (1 - n u),  |fl(sum a_i b_i) - sum a_i b_i| <= gamma_n sum |a_i b_i|.

  shrink  u[t] = pro(x)[t] A[ids[t]]^T              gamma(C)          on |pro(x)| |A|^T
  expand  y[t] = s + scale u[t] B[ids[t]]^T + res   gamma(C + r + 3)  on |s| + |scale| |u| |B|^T + |res|

where s = pro(x) W^T is a sum the kernel forms itself, so ``|s|`` is its majorant |pro(x)| |W|^T (as
every kernel-formed sum in tests/lora_oracle.py; the absolute value of a cancelling sum bounds
nothing), while ``u`` is an operand of the expand — the fp32 tensor the kernel is given — and enters
as it is. n = C + r + 3: the two chains, the scale, the residual add, the rounding of pro(x).

The prologues are rounded too: an rmsnorm row is (sum of C squares, a division, a square root, two
products), a swiglu element (an exponential, an add, a division, two products). The kernels' own
depth is far below n — a lane's chain is 4 ceil(C / 256) fmaf long, the butterfly 6 adds, the
rmsnorm's sum of squares the same again at half weight (the square root), the elementwise roundings
below 8 u — under 50 u for C <= 2048, against n u >= 96 u at the smallest C a prologue is tested
with. Nothing here is fitted to any output: tests/test_adapter_generate_cpu.py asserts that plain
torch fp32 meets the bound on every case before a kernel is judged by it.

An id outside [0, R) means "no adapter": a zero row of u, and y = s + res.
"""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def _f64(t):
    return t.detach().cpu().double().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float64)


class Q:
    """value and absolute error bound of its fp32 counterpart."""

    def __init__(self, v, e):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)


def prologue(x, pro="none", gain=None, eps=1e-6):
    x = _f64(x)
    if pro == "rmsnorm":
        return x / np.sqrt((x * x).mean(-1, keepdims=True) + float(np.float32(eps))) * _f64(gain)
    if pro == "swiglu":
        a, b = x[:, :x.shape[1] // 2], x[:, x.shape[1] // 2:]
        return a / (1.0 + np.exp(-a)) * b
    assert pro == "none"
    return x


def _slots(ids, R):
    ids = np.asarray(ids.detach().cpu().numpy() if hasattr(ids, "detach") else ids, dtype=np.int64)
    return [int(i) if 0 <= int(i) < R else None for i in ids]


def shrink(x, A, ids, pro="none", gain=None, eps=1e-6):
    """x [T, C] ([T, 2C] for swiglu), A [R, r, C], ids [T] -> u [T, r] as Q."""
    xp, A = prologue(x, pro, gain, eps), _f64(A)
    T, C = xp.shape
    r = A.shape[1]
    u, mu = np.zeros((T, r)), np.zeros((T, r))
    for t, k in enumerate(_slots(ids, A.shape[0])):
        if k is not None:
            u[t] = A[k] @ xp[t]
            mu[t] = np.abs(A[k]) @ np.abs(xp[t])
    return Q(u, gamma(C) * mu)


def expand(x, w, u, B, ids, scale, res=None, pro="none", gain=None, eps=1e-6):
    """y [T, K] = pro(x) w^T + scale u[t] B[ids[t]]^T (+ res) as Q; u [T, r] is an operand."""
    xp, w, u, B = prologue(x, pro, gain, eps), _f64(w), _f64(u), _f64(B)
    s = float(np.float32(scale))
    C, r = w.shape[1], B.shape[2]
    y, m = xp @ w.T, np.abs(xp) @ np.abs(w).T
    for t, k in enumerate(_slots(ids, B.shape[0])):
        if k is not None:
            y[t] += s * (B[k] @ u[t])
            m[t] += abs(s) * (np.abs(B[k]) @ np.abs(u[t]))
    if res is not None:
        y, m = y + _f64(res), m + np.abs(_f64(res))
    return Q(y, gamma(C + r + 3) * m)


def merged64(w, a, b, scale):
    """The merged twin of one adapted weight: W + scale B A in float64. w [N, D], a [r, D], b [N, r]."""
    return _f64(w) + float(scale) * (_f64(b) @ _f64(a))


def ratio(got, want: Q):
    """worst |got - value| / bound over the array (0 / 0 counts as 0, x / 0 as inf; NaN as inf)."""
    err = np.abs(_f64(got) - want.v)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / want.e)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0
