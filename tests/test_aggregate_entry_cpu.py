"""``fl.aggregate.aggregate_into`` is the one place that knows how an aggregator is called. Held here
bit for bit to the three call sequences the algorithms spelled out before it existed (FedAvg, FedAvg
behind a server optimizer, FedSGD), written out literally below, for every calling convention: the
mean, the clipped mean with a centre, and the robust rules that act on updates. K = 5 clients of
P = 37 coordinates on one rank (an odd P: no multiple of any shard or quad width)."""
import pytest
import torch

from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.fl.server_opt import make_server_opt
from ddl25spring_amd.runtime.dist import DistContext

K, P, LR = 5, 37, 0.1
AGGS = {
    "mean": lambda: A.MeanAggregator(),
    "clipped_mean": lambda: A.ClippedMean(clip=1.0),  # clips the three longest of the updates below
    "median": lambda: A.Median(),
    "trimmed_mean": lambda: A.TrimmedMean(1),
    "krum": lambda: A.Krum(f=1, m=1),
}


def _inputs():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(P, generator=g)
    scale = torch.tensor([0.05, 0.1, 0.2, 0.4, 0.8]).reshape(K, 1)
    rows = w + scale * torch.randn(K, P, generator=g)
    n = torch.tensor([30.0, 10.0, 25.0, 15.0, 20.0])
    return w, rows, n / n.sum(), [K], list(range(K))


def _legacy_fedavg(agg, ctx, rows, coeffs, w_global, counts, keys):
    if getattr(agg, "takes_center", False):
        agg(ctx, rows, coeffs, w_global, center=w_global, counts=counts)
    elif not getattr(agg, "needs_all", False):
        agg(ctx, rows, coeffs, w_global)
    else:
        upd = rows - w_global
        res = agg(ctx, upd, counts, w_global.numel(), keys=keys)
        w_global.add_(res)


def _legacy_server_opt(agg, opt, ctx, rows, coeffs, w_global, counts, keys):
    target = torch.empty_like(w_global)
    if getattr(agg, "takes_center", False):
        agg(ctx, rows, coeffs, target, center=w_global, counts=counts)
        opt.step(w_global, target, False)
    elif not getattr(agg, "needs_all", False):
        agg(ctx, rows, coeffs, target)
        opt.step(w_global, target, False)
    else:
        upd = rows - w_global
        target.copy_(agg(ctx, upd, counts, w_global.numel(), keys=keys))
        opt.step(w_global, target, True)


def _legacy_fedsgd(agg, ctx, grads, coeffs, g_global, w_global, counts, keys):
    if getattr(agg, "takes_center", False):
        agg(ctx, grads, coeffs, g_global, center=None, counts=counts)
    elif not getattr(agg, "needs_all", False):
        agg(ctx, grads, coeffs, g_global)
    else:
        g_global.copy_(agg(ctx, grads, counts, w_global.numel(), keys=keys))
    w_global.add_(g_global, alpha=-LR)


def _fedavg(make):
    """-> (tensors through the entry point, the same through the legacy sequence, the start)"""
    w, rows, coeffs, counts, keys = _inputs()
    ctx = DistContext()
    new, old = w.clone(), w.clone()
    is_update = A.aggregate_into(make(), ctx, rows, coeffs, new, center=new, counts=counts, keys=keys)
    assert is_update is False
    _legacy_fedavg(make(), ctx, rows, coeffs, old, counts, keys)
    return [new], [old], w


def _server_opt(make):
    w, rows, coeffs, counts, keys = _inputs()
    ctx = DistContext()
    new, old = w.clone(), w.clone()
    opt_new, opt_old = make_server_opt("fedadam"), make_server_opt("fedadam")
    for r in range(2):  # the second round steps moments that are no longer their initial values
        moved = rows + 0.01 * r
        target = torch.empty_like(new)
        is_update = A.aggregate_into(make(), ctx, moved, coeffs, target, center=new, counts=counts, keys=keys,
                                     as_update=True)
        assert is_update is bool(getattr(make(), "needs_all", False))  # the robust rules hand over the delta
        opt_new.step(new, target, is_update)
        _legacy_server_opt(make(), opt_old, ctx, moved, coeffs, old, counts, keys)
    return [new, opt_new.m, opt_new.v], [old, opt_old.m, opt_old.v], w


def _fedsgd(make):
    w, rows, coeffs, counts, keys = _inputs()
    ctx = DistContext()
    grads = rows - w  # any K vectors do: FedSGD hands the gradients over as the updates
    new, old = w.clone(), w.clone()
    g_new, g_old = torch.zeros(P), torch.zeros(P)
    A.aggregate_into(make(), ctx, grads, coeffs, g_new, center=None, counts=counts, keys=keys)
    new.add_(g_new, alpha=-LR)
    _legacy_fedsgd(make(), ctx, grads, coeffs, g_old, old, counts, keys)
    return [new, g_new], [old, g_old], w


@pytest.mark.parametrize("route", [_fedavg, _server_opt, _fedsgd], ids=["fedavg", "server_opt", "fedsgd"])
@pytest.mark.parametrize("name", AGGS)
def test_entry_point_equals_legacy_call_sequence(name, route):
    new, old, start = route(AGGS[name])
    assert not torch.equal(new[0], start)  # the server model moved
    for a, b in zip(new, old):
        assert torch.equal(a, b)
