"""``ops.SpecAugmentFn`` / ``ops.spec_augment``: the autograd wrapper around re2e_spec_augment_fwd / _bwd (csrc/specaug.hip; the plan's layout
and ranges are stated in include/re2e.h).  It carries no parameters, so none of ops.py's parameter-gradient protocol applies to it.  ops.py
imports this module at its end; its helpers are taken from it at call time, so neither import order fails."""
import torch

from . import lib
from .lib import call


class SpecAugmentFn(torch.autograd.Function):
    """SpecAugment on (R, Tp, F) features: time warp, frequency and time masks in one launch, dx = J^T dy in one launch
    (csrc/specaug.hip; the plan's layout is stated in include/re2e.h).  ``plan_dev``: the (R, P) int32 plan on x's device."""

    @staticmethod
    def forward(ctx, x, plan_dev, nF, nT):
        from . import ops
        ops._need_gpu(x)
        x = ops._f32(x)
        R, Tp, F = x.shape
        y = ops.empty((R, Tp, F), x)
        call('re2e_spec_augment_fwd', x.data_ptr(), plan_dev.data_ptr(), R, Tp, F, nF, nT, y.data_ptr())
        ctx.plan_dev, ctx.dims = plan_dev, (R, Tp, F, nF, nT)
        return y

    @staticmethod
    def backward(ctx, dy):
        R, Tp, F, nF, nT = ctx.dims
        from . import ops
        dy = ops._f32(dy)
        dx = ops.empty((R, Tp, F), dy)
        call('re2e_spec_augment_bwd', dy.data_ptr(), ctx.plan_dev.data_ptr(), R, Tp, F, nF, nT, dx.data_ptr())
        return dx, None, None, None


def spec_augment(x, plan, nF=None):
    """y = masks(warp(x)) for x (R, Tp, F) on the GPU.  ``plan``: a ``data.spec_augment.Plan``, or a HOST (R, 3 + 2 nF + 2 nT) integer array
    with ``nF`` named.  It is validated on the host against the ranges of include/re2e.h and uploaded through pinned memory on the current
    stream (no host synchronisation); the backward runs on the forward's stream, behind that copy."""
    from .data import spec_augment as sa
    from .model.e2e_common import host_to_dev
    if isinstance(plan, sa.Plan):
        plan, nF = plan.rows, plan.nF
    if nF is None:
        raise lib.Re2eError('ops.spec_augment: a bare plan array needs nF (the number of frequency masks per row)')
    from . import ops
    ops._need_gpu(x)
    if x.dim() != 3:
        raise lib.Re2eError('ops.spec_augment: x is (R, Tp, F), got %r' % (tuple(x.shape),))
    try:
        rows, nT = sa.validate_plan(plan, x.shape[1], x.shape[2], nF)
    except ValueError as e:
        raise lib.Re2eError('ops.spec_augment: %s' % e)
    if rows.shape[0] != x.shape[0]:
        raise lib.Re2eError('ops.spec_augment: %d plan rows for %d feature rows' % (rows.shape[0], x.shape[0]))
    return SpecAugmentFn.apply(x, host_to_dev(rows, x.device), int(nF), nT)
