"""Float64 oracle of SCAFFOLD's local step and round-end control-variate update
(csrc/kernels/scaffold.hip), with an elementwise first-order error bound and an op-by-op
``np.float32`` emulation.

numpy on the host, written from the definitions (Karimireddy et al. 2020, Algorithm 1, option II);
it shares no code with the kernels or their torch twins, both of which are checked against it. The
error-propagating arithmetic ``Q`` is the one of tests/fedopt_oracle.py: inputs carry no error, every
add, subtract and multiply of the fp32 code is allowed u |result| (u = 2^-24, correctly rounded), and
the allowances are propagated to first order. The hyper-parameters enter as the fp32 values the
kernels receive; ``1 - dampening`` is formed in fp32, which is part of the definition.

The round-end update walks the slots in order, as the definition's sum is written:

    t_g = (x - y_g) * k_g;  delta_g = t_g - c;  bank_g' = bank_g + delta_g;  acc_g = acc_{g-1} + delta_g * inv_n

so dc = acc_{G-1} carries G product roundings and G adds, each bounded through ``Q``; acc_{-1} = 0. A
coordinate whose delta_g is NaN / Inf contributes nothing and leaves bank_g (bound 0 there).
Nothing here is fitted to any output: ``emulate_*`` shows the bound is met by straightforward fp32
code, and tests/test_scaffold_cpu.py asserts that on every case before a kernel is judged by it.
"""
import numpy as np

from fedopt_oracle import Q, U, _f32, _f64, add, mul, one_minus32, ratio, s32, sub  # noqa: F401


def _ids(slot_client):
    return [int(i) for i in (slot_client.tolist() if hasattr(slot_client, "tolist") else slot_client)]


# ------------------------------------------------------------------------------------- local step
def scaffold_step(p, g, mom, c, bank, slot_client, lr, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False,
                  first_step=False, grad_scale=1.0):
    """Rows p, g, mom [G, P] (mom may be None), c [P], bank [N, P], slot_client [G] -> (p1, m1) as
    Q; m1 None without momentum. d = g * grad_scale + wd * p + (c - bank[slot_client[row]]);
    momentum, dampening, nesterov as torch.optim.SGD; p1 = p - lr * d."""
    p, g = Q(_f64(p)), Q(_f64(g))
    corr = sub(Q(_f64(c)[None, :]), Q(_f64(bank)[_ids(slot_client)]))
    lr, wd, mo, gs = (Q(s32(s)) for s in (lr, wd, momentum, grad_scale))
    d = add(add(mul(g, gs), mul(wd, p)), corr)
    m1 = None
    if momentum != 0.0:
        if first_step:
            m1 = d
        else:
            m1 = add(mul(mo, Q(_f64(mom))), mul(Q(one_minus32(dampening)), d))
        d = add(d, mul(mo, m1)) if nesterov else m1
    return sub(p, mul(lr, d)), m1


def emulate_scaffold_step(p, g, mom, c, bank, slot_client, lr, wd=0.0, momentum=0.0, dampening=0.0,
                          nesterov=False, first_step=False, grad_scale=1.0):
    f = np.float32
    p, g = _f32(p), _f32(g)
    corr = _f32(c)[None, :] - _f32(bank)[_ids(slot_client)]
    lr, wd, mo, gs = f(lr), f(wd), f(momentum), f(grad_scale)
    d = (g * gs + wd * p) + corr
    m1 = None
    if momentum != 0.0:
        m1 = d if first_step else mo * _f32(mom) + (f(1.0) - f(dampening)) * d
        d = d + mo * m1 if nesterov else m1
    p1 = p - lr * d
    assert p1.dtype == np.float32
    return p1, m1


# -------------------------------------------------------------------------------- round-end update
def finish(rows, x, c, bank, slot_client, inv_klr, inv_n):
    """-> (bank1 [G, P] as Q: the new rows of the slots' clients, dc as Q, c1 = c + dc as Q, ok
    [G, P]: the finite-delta mask)."""
    y, bank = _f64(rows), _f64(bank)
    x, c0 = Q(_f64(x)), Q(_f64(c))
    k, n_ = _f64(_f32(inv_klr)), Q(s32(inv_n))
    acc = Q(np.zeros_like(x.v))
    bv, be, oks = [], [], []
    with np.errstate(all="ignore"):
        for g, cl in enumerate(_ids(slot_client)):
            t = mul(sub(x, Q(y[g])), Q(k[g]))
            delta = sub(t, c0)
            ok = np.isfinite(delta.v)
            delta = Q(np.where(ok, delta.v, 0.0), np.where(ok, delta.e, 0.0))
            b1 = add(Q(bank[cl]), delta)
            a1 = add(acc, mul(delta, n_))
            bv.append(np.where(ok, b1.v, bank[cl]))
            be.append(np.where(ok, b1.e, 0.0))
            acc = Q(np.where(ok, a1.v, acc.v), np.where(ok, a1.e, acc.e))
            oks.append(ok)
    return Q(np.stack(bv), np.stack(be)), acc, add(c0, acc), np.stack(oks)


def emulate_finish(rows, x, c, bank, slot_client, inv_klr, inv_n):
    """The same update op by op in np.float32 -> (bank1 [G, P], dc, c1)."""
    f = np.float32
    y, x, c, bank, k = _f32(rows), _f32(x), _f32(c), _f32(bank), _f32(inv_klr)
    inv_n = f(inv_n)
    acc = np.zeros_like(x)
    out = []
    with np.errstate(all="ignore"):
        for g, cl in enumerate(_ids(slot_client)):
            delta = (x - y[g]) * k[g] - c
            ok = np.isfinite(delta)
            delta = np.where(ok, delta, f(0.0))
            out.append(np.where(ok, bank[cl] + delta, bank[cl]))
            acc = np.where(ok, acc + delta * inv_n, acc)
    c1 = c + acc
    assert acc.dtype == np.float32 and c1.dtype == np.float32 and out[0].dtype == np.float32
    return np.stack(out), acc, c1
