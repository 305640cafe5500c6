"""Float64 oracle of the FedProx local step and the FedOpt server step (csrc/kernels/fedopt.hip),
with an elementwise first-order error bound and an op-by-op ``np.float32`` emulation.

numpy on the host, written from the definitions; it shares no code with the kernels or their torch
twins (``ddl25spring_amd.ops.reference``), both of which are checked against it.

The oracle takes the SAME fp32 inputs as the code under test (w, x or the client rows, m, v; the
hyper-parameters rounded to fp32; ``1 - beta`` and ``1 - dampening`` formed in fp32, which is part of
the definition) and evaluates one step in float64. Every quantity is carried as a pair
(value, err): ``err`` bounds |fp32 result - value| to first order under the allowances

  * add, subtract, multiply : u |result|,   u = 2^-24 (correctly rounded);
  * divide, sqrtf           : 2u |result|   (not assumed correctly rounded);
  * inputs                  : 0;

propagated through the formulas by the usual rules (``Q`` below). For the fused kernel the
weighted sum x = sum_g c_g r_g enters with err = G u sum_g |c_g r_g| (G product roundings and G - 1
adds of partial sums bounded by the mass; the shape of ``clip_oracle.sum_bound``), whatever the
order of the adds. Yogi's sign(v - delta^2) is discontinuous: where |v - delta^2| is within its own
err the fp32 sign may differ from the exact one, and 2 (1 - b2) delta^2 is added to v's err there.
Nothing here is fitted to any output: ``emulate_*`` shows the bound is met by straightforward fp32
code, and tests/test_fedopt_cpu.py asserts that on every case before a kernel is judged by it.
"""
import numpy as np

U = 2.0 ** -24
KINDS = ("sgdm", "adagrad", "adam", "yogi")


def _f64(t):
    return t.detach().cpu().double().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float64)


def _f32(t):
    return t.detach().cpu().float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def s32(x):
    """A hyper-parameter as the fp32 value the kernels receive, held in float64."""
    return float(np.float32(x))


def one_minus32(x):
    """1 - x formed in fp32."""
    return float(np.float32(1.0) - np.float32(x))


class Q:
    """value and first-order absolute error bound of its fp32 counterpart."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy() if np.ndim(v) else \
            np.asarray(e, dtype=np.float64)


def add(a, b):
    v = a.v + b.v
    return Q(v, a.e + b.e + U * np.abs(v))


def sub(a, b):
    v = a.v - b.v
    return Q(v, a.e + b.e + U * np.abs(v))


def mul(a, b):
    v = a.v * b.v
    return Q(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + U * np.abs(v))


def div(a, b):
    v = a.v / b.v
    return Q(v, a.e / np.abs(b.v) + np.abs(a.v) * b.e / (b.v * b.v) + 2 * U * np.abs(v))


def sqrt(a):
    v = np.sqrt(a.v)
    # sqrt is concave: the largest deviation over [a - e, a + e] is towards a - e (clamped at 0)
    return Q(v, v - np.sqrt(np.maximum(a.v - a.e, 0.0)) + 2 * U * v)


# ------------------------------------------------------------------------------- server optimizers
def _server(kind, w, x, m, v, x_is_delta, lr, beta1, beta2, tau):
    """w, m, v: float64 arrays of fp32 values; x: Q. -> (w1, m1, v1) as Q, finite mask."""
    assert kind in KINDS
    w, m, v = Q(w), Q(m), Q(v)
    lr, b1, b2, tau_ = Q(s32(lr)), Q(s32(beta1)), Q(s32(beta2)), Q(s32(tau))
    omb1, omb2 = Q(one_minus32(beta1)), Q(one_minus32(beta2))
    with np.errstate(all="ignore"):
        d = x if x_is_delta else sub(x, w)
        ok = np.isfinite(d.v)
        d = Q(np.where(ok, d.v, 0.0), np.where(ok, d.e, 0.0))
        if kind == "sgdm":
            m1 = add(mul(b1, m), d)
            w1 = add(w, mul(lr, m1))
            v1 = v
        else:
            m1 = add(mul(b1, m), mul(omb1, d))
            if kind == "adagrad":
                v1 = add(v, mul(d, d))
            elif kind == "adam":
                v1 = add(mul(b2, v), mul(mul(omb2, d), d))
            else:
                d2 = mul(d, d)
                diff = sub(v, d2)
                t = mul(omb2, d2)
                v1 = sub(v, Q(t.v * np.sign(diff.v), t.e))
                v1.e = v1.e + np.where(np.abs(diff.v) <= diff.e, 2.0 * np.abs(t.v), 0.0) * (diff.e > 0)
            w1 = add(w, div(mul(lr, m1), add(sqrt(v1), tau_)))
    out = []
    for new, old in ((w1, w), (m1, m), (v1, v)):
        out.append(Q(np.where(ok, new.v, old.v), np.where(ok, new.e, 0.0)))
    return out[0], out[1], out[2], ok


def server_step(kind, w, x, m, v, x_is_delta, lr, beta1=0.9, beta2=0.99, tau=1e-3):
    """One step from fp32 inputs -> (w1, m1, v1) as Q (value, bound) and the mask of coordinates
    with a finite delta (the others keep w, m, v, bound 0). v may be None for sgdm."""
    w, x, m = _f64(w), _f64(x), _f64(m)
    v = np.zeros_like(w) if v is None else _f64(v)
    return _server(kind, w, Q(x), m, v, x_is_delta, lr, beta1, beta2, tau)


def weighted_sum(rows, coeff):
    """-> Q of x = sum_g c_g r_g in float64 with err G u sum_g |c_g r_g|."""
    r, c = _f64(rows), _f64(_f32(coeff))
    terms = c[:, None] * r
    return Q(terms.sum(0), r.shape[0] * U * np.abs(terms).sum(0))


def server_step_rows(kind, rows, coeff, w, m, v, lr, beta1=0.9, beta2=0.99, tau=1e-3, x_is_delta=False):
    w, m = _f64(w), _f64(m)
    v = np.zeros_like(w) if v is None else _f64(v)
    return _server(kind, w, weighted_sum(rows, coeff), m, v, x_is_delta, lr, beta1, beta2, tau)


def emulate_server_step(kind, w, x, m, v, x_is_delta, lr, beta1=0.9, beta2=0.99, tau=1e-3):
    """The same step op by op in np.float32 (each operation rounded on its own)."""
    f = np.float32
    w, x, m = _f32(w).copy(), _f32(x), _f32(m).copy()
    v = np.zeros_like(w) if v is None else _f32(v).copy()
    lr, b1, b2, tau = f(lr), f(beta1), f(beta2), f(tau)
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(all="ignore"):
        d = x if x_is_delta else x - w
        ok = np.isfinite(d)
        d = np.where(ok, d, f(0.0))
        if kind == "sgdm":
            m1 = b1 * m + d
            w1 = w + lr * m1
            v1 = v
        else:
            m1 = b1 * m + omb1 * d
            if kind == "adagrad":
                v1 = v + d * d
            elif kind == "adam":
                v1 = b2 * v + (omb2 * d) * d
            else:
                d2 = d * d
                v1 = v - (omb2 * d2) * np.sign(v - d2)
            w1 = w + (lr * m1) / (np.sqrt(v1) + tau)
    for a in (w1, m1, v1):
        assert a.dtype == np.float32
    return np.where(ok, w1, w), np.where(ok, m1, m), np.where(ok, v1, v)


def emulate_weighted_sum(rows, coeff):
    """weighted_sum_kernel's order in np.float32: from 0, products rounded, added in row order."""
    r, c = _f32(rows), _f32(coeff)
    acc = np.zeros(r.shape[1], dtype=np.float32)
    for g in range(r.shape[0]):
        acc = acc + c[g] * r[g]
    return acc


# ----------------------------------------------------------------------------------- FedProx step
def prox_step(p, g, mom, a, lr, mu, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False, first_step=False,
              grad_scale=1.0):
    """Rows p, g, mom [G, P] (mom may be None), anchor a [P] -> (p1, m1) as Q; m1 None without
    momentum. d = g * grad_scale + wd * p + mu * (p - a); momentum, dampening, nesterov as
    torch.optim.SGD; p1 = p - lr * d."""
    p, g, a = Q(_f64(p)), Q(_f64(g)), Q(_f64(a)[None, :])
    lr, mu, wd, mo, gs = (Q(s32(s)) for s in (lr, mu, wd, momentum, grad_scale))
    d = add(add(mul(g, gs), mul(wd, p)), mul(mu, sub(p, a)))
    m1 = None
    if momentum != 0.0:
        if first_step:
            m1 = d
        else:
            m1 = add(mul(mo, Q(_f64(mom))), mul(Q(one_minus32(dampening)), d))
        d = add(d, mul(mo, m1)) if nesterov else m1
    return sub(p, mul(lr, d)), m1


def emulate_prox_step(p, g, mom, a, lr, mu, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False,
                      first_step=False, grad_scale=1.0):
    f = np.float32
    p, g, a = _f32(p), _f32(g), _f32(a)[None, :]
    lr, mu, wd, mo, gs = f(lr), f(mu), f(wd), f(momentum), f(grad_scale)
    d = (g * gs + wd * p) + mu * (p - a)
    m1 = None
    if momentum != 0.0:
        m1 = d if first_step else mo * _f32(mom) + (f(1.0) - f(dampening)) * d
        d = d + mo * m1 if nesterov else m1
    p1 = p - lr * d
    assert p1.dtype == np.float32
    return p1, m1


def ratio(got, want: Q):
    """worst |got - value| / bound over the array (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(_f64(got) - want.v)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / want.e)
    return float(np.max(r)) if r.size else 0.0
