"""re2e_conv3x3_wino_valid (csrc/winograd.hip): the fused Winograd F(2x2,3x3) forward over a padded image batch in which image n IS an image
of valid[n] rows -- against the float64 reference of tests/refs64_conv.py on the CROPPED images, through the C ABI, in the manner of
tests/test_conv_kernels_gpu.py: outputs and workspace prefilled with NaN, guard floats around every output that must come back unchanged,
every call twice on fresh buffers with bit-equal results, the bars of refs64_conv.BARS with the fp32 CPU yardstick (the Winograd evaluation
in float32) held to an eighth of them.

Shapes: W = 16 selects the 16 x 8 patch and W = 8 the 8 x 16 patch; (C, Cout) in (8, 64), (64, 64), (64, 128), (128, 128) are the per-lane,
the 64-channel and the general LDS-staged kernels with one and two channel groups; H = 40, N = 6, valid = 40, 33, 17, 16, 9, 1: the full
height, an odd length, one past / at an edge of the 16-row patch, one past an edge of the 8-row patch, a single row.  With and without the
fused pool; the input rows >= valid[n] hold NaN in one run and 1e30 in another.  What is compared: rows < valid[n] (pooled: < ceil(valid[n]
/ 2)), all finite, within the bar of float64 (index bytes: the float64 ones except between near-ties), AND equal bit for bit to
re2e_conv3x3_wino run on the cropped image alone -- a tile's arithmetic depends neither on the patch it lies in nor on the image height.
Rows beyond are unspecified and not looked at.  A second test chains conv1_2 + pool -> conv2_1 -> conv2_2 + pool with the lengths halving
behind the pool and every intermediate buffer prefilled with NaN; a third the argument checks.  GPU only."""
import functools

import pytest
import torch

import refs64_conv as R
from test_conv_kernels_gpu import DEV, NAN, _Out, _check_index_bytes, _in, _ws

pytestmark = pytest.mark.gpu

H, N, VALID = 40, 6, (40, 33, 17, 16, 9, 1)
CHANNELS = ((8, 64), (64, 64), (64, 128), (128, 128))
FAM = 'wino3x3'


def _lib():
    from robust_e2e_gan_amd import lib
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    return lib


def _rows(pool, v):
    return (v + 1) // 2 if pool else v


def _layer(x, w, b, pool, dtype):
    """relu(conv(x) + b) of ONE image (1, v, W, C), optionally ceil-mode pooled -> (values, index bytes or None).  float64: the tap-by-tap
    reference; float32: the fp32 Winograd evaluation (the yardstick of the family)."""
    if dtype == torch.float64:
        y = R.conv_fwd(x, w, b, 1, 1, R.ACT_RELU)
    else:
        y = torch.clamp(R.wino_fwd(x, w, 1, torch.float32) + b, min=0)
    return R.relu_pool(y) if pool else (y, None)


@functools.lru_cache(maxsize=None)
def _case(W, C, Cout):
    """Inputs and, per image, the float64 reference and the fp32 yardstick on the cropped image, with and without the pool."""
    g = torch.Generator().manual_seed(7 * W + 131 * C + Cout)
    x = R.rnd(g, N, H, W, C)
    w = R.rnd(g, Cout, C, 3, 3, scale=(9 * C) ** -0.5)
    b = R.rnd(g, Cout, scale=0.3)
    ref = {pool: [(_layer(x[n:n + 1, :v], w, b, pool, torch.float64), _layer(x[n:n + 1, :v], w, b, pool, torch.float32)[0])
                  for n, v in enumerate(VALID)] for pool in (False, True)}
    return x, w, b, ref


def _guarded(o, tag):
    """The output between its guards, which must be untouched (rows beyond a valid height may still hold the NaN prefill)."""
    torch.cuda.synchronize()
    s = o.store.cpu()
    assert (s[:o.off] == o.fill).all() and (s[o.off + o.n:] == o.fill).all(), '%s: a guard beside the output was written' % tag
    return s[o.off:o.off + o.n].view(o.t.shape).clone()


def _launch(lib, name, x, w, b, Hh, pool, valid, tag):
    """One call on fresh buffers -> (values, index bytes or None) on the CPU."""
    n, _, W, C = x.shape
    Cout = w.shape[0]
    shape = (n, (Hh + 1) // 2, (W + 1) // 2, Cout) if pool else (n, Hh, W, Cout)
    out = _Out(shape)
    idx = _Out(shape, dtype=torch.uint8) if pool else None
    ws, wsb = _ws(lib.query('re2e_conv3x3_wino_workspace_bytes', C, Cout))
    tail = (ws.data_ptr(), wsb) if valid is None else (valid.data_ptr(), ws.data_ptr(), wsb)
    lib.call(name, x.data_ptr(), n, Hh, W, C, w.data_ptr(), Cout, 0, b.data_ptr(), 1, None, None if pool else out.ptr(), out.ptr() if pool else None,
             idx.ptr() if pool else None, *tail)
    return _guarded(out, tag), (_guarded(idx, tag + ' (index bytes)') if pool else None)


@functools.lru_cache(maxsize=None)
def _alone(W, C, Cout, pool):
    """re2e_conv3x3_wino on every cropped image by itself."""
    lib = _lib()
    x, w, b, _ = _case(W, C, Cout)
    wd, bd = _in(w), _in(b)
    res = []
    for n, v in enumerate(VALID):
        y, i = _launch(lib, 're2e_conv3x3_wino', _in(x[n:n + 1, :v]), wd, bd, v, pool, None, 'alone')
        assert torch.isfinite(y).all()
        res.append((y, i))
    return res


@pytest.mark.parametrize('beyond', [NAN, 1e30], ids=['nan', '1e30'])
@pytest.mark.parametrize('pool', [False, True], ids=['full', 'pool'])
@pytest.mark.parametrize('C,Cout', CHANNELS)
@pytest.mark.parametrize('W', [16, 8])
def test_valid_height_against_float64_and_the_cropped_image(W, C, Cout, pool, beyond):
    lib = _lib()
    x, w, b, ref = _case(W, C, Cout)
    tag = 'valid W%d %d->%d %s beyond=%s' % (W, C, Cout, 'pool' if pool else 'full', beyond)
    xin = x.clone()
    for n, v in enumerate(VALID):
        xin[n, v:] = beyond
    valid = torch.tensor(VALID, dtype=torch.int32).to(DEV)
    runs = [_launch(lib, 're2e_conv3x3_wino_valid', _in(xin), _in(w), _in(b), H, pool, valid, tag) for _ in range(2)]
    alone = _alone(W, C, Cout, pool)
    q = 'pool' if pool else 'y'
    bar = R.BARS[q, FAM]
    assert bar <= R.BAR_CAP
    got, f64, yard = [], [], []
    for n, v in enumerate(VALID):
        r = _rows(pool, v)
        (y0, i0), (y1, i1) = runs[0], runs[1]
        a = y0[n:n + 1, :r]
        assert torch.isfinite(a).all(), '%s image %d: rows below the valid height are not finite (or were left unwritten)' % (tag, n)
        assert torch.equal(a, y1[n:n + 1, :r]), '%s image %d: two runs on fresh buffers differ' % (tag, n)
        assert torch.equal(a, alone[n][0]), '%s image %d: not bit-equal to re2e_conv3x3_wino on the cropped image (max diff %.3e)' % (
            tag, n, (a - alone[n][0]).abs().max().item())
        (v64, idx64), y32 = ref[pool][n]
        if pool:
            ib = i0[n:n + 1, :r]
            assert (ib <= 4).all() and torch.equal(ib, i1[n:n + 1, :r]) and torch.equal(ib, alone[n][1]), '%s image %d: index bytes' % (tag, n)
            row = R._row(None, R.FWD, 1, v, W, C, Cout, 3, 1, R.ACT_RELU, R.F_BIAS | R.F_POOL)
            _check_index_bytes('%s image %d' % (tag, n), row, dict(x=x[n:n + 1, :v], w=w, b=b), ib, v64, idx64, bar)
        got.append(a.reshape(-1))
        f64.append(v64.reshape(-1))
        yard.append(y32.reshape(-1))
    got, f64, yard = torch.cat(got), torch.cat(f64), torch.cat(yard)
    cpu, err = R.rel_err(yard, f64), R.rel_err(got, f64)
    print('ERR %-44s %-4s %-7s hip %.2e  fp32-cpu %.2e  bar %.0e' % (tag, q, FAM, err, cpu, bar))
    assert cpu <= bar / 8, 'input too hard for the bar: the fp32 CPU yardstick of %s is %.3e from float64, the bar is %.1e' % (tag, cpu, bar)
    assert err <= bar, '%s: HIP is %.3e of the max from float64 (bar %.1e, fp32 yardstick on the CPU: %.3e)' % (tag, err, bar, cpu)


def test_valid_height_chain():
    """conv1_2 + pool -> conv2_1 -> conv2_2 + pool at N = 3, H = 21, W = 8, 64 -> 64 -> 128 -> 128, valid = 21, 14, 5: the lengths halve behind
    the pool (11, 7, 3 rows into conv2_1 and conv2_2; 6, 4, 2 pooled rows at the end), every intermediate buffer holds NaN before its producer
    runs and keeps it in the rows no producer writes.  The final pooled rows below ceil(ceil(v / 2) / 2) are finite and within the pool bar of
    the float64 chain on the cropped images."""
    lib = _lib()
    Nn, Hh, W, valid = 3, 21, 8, (21, 14, 5)
    g = torch.Generator().manual_seed(2105)
    x = R.rnd(g, Nn, Hh, W, 64).clamp(min=0)                   # a ReLU output, as conv1_1 leaves it
    ws_ = [(R.rnd(g, co, ci, 3, 3, scale=(9 * ci) ** -0.5), R.rnd(g, co, scale=0.3)) for ci, co in ((64, 64), (64, 128), (128, 128))]
    pools = (True, False, True)

    def chain(img, dtype):
        h = img
        for (w, b), pool in zip(ws_, pools):
            h = _layer(h.to(dtype), w, b, pool, dtype)[0]
        return h

    xin = x.clone()
    for n, v in enumerate(valid):
        xin[n, v:] = NAN
    v1 = torch.tensor(valid, dtype=torch.int32).to(DEV)
    v2 = torch.tensor([(v + 1) // 2 for v in valid], dtype=torch.int32).to(DEV)
    H2, W2 = (Hh + 1) // 2, (W + 1) // 2
    hd = _in(xin)
    wd = [(_in(w), _in(b)) for w, b in ws_]
    outs = []
    for k, (pool, hh, ww, vv) in enumerate(((True, Hh, W, v1), (False, H2, W2, v2), (True, H2, W2, v2))):
        Cout, C = ws_[k][0].shape[0], ws_[k][0].shape[1]
        shape = (Nn, (hh + 1) // 2, (ww + 1) // 2, Cout) if pool else (Nn, hh, ww, Cout)
        out = _Out(shape)                                       # NaN before its producer runs
        idx = _Out(shape, dtype=torch.uint8) if pool else None
        wsp, wsb = _ws(lib.query('re2e_conv3x3_wino_workspace_bytes', C, Cout))
        lib.call('re2e_conv3x3_wino_valid', hd.data_ptr(), Nn, hh, ww, C, wd[k][0].data_ptr(), Cout, 0, wd[k][1].data_ptr(), 1, None,
                 None if pool else out.ptr(), out.ptr() if pool else None, idx.ptr() if pool else None, vv.data_ptr(), wsp.data_ptr(), wsb)
        outs.append((out, idx, wsp))
        hd = out.t
    final = _guarded(outs[2][0], 'chain')
    for k in range(2):
        _guarded(outs[k][0], 'chain layer %d' % k)
    bar = R.BARS['pool', FAM]
    got, f64, yard = [], [], []
    for n, v in enumerate(valid):
        r = ((v + 1) // 2 + 1) // 2
        a = final[n:n + 1, :r]
        assert torch.isfinite(a).all(), 'chain image %d: final pooled rows are not finite' % n
        got.append(a.reshape(-1))
        f64.append(chain(x[n:n + 1, :v], torch.float64).reshape(-1))
        yard.append(chain(x[n:n + 1, :v], torch.float32).reshape(-1))
        assert f64[-1].numel() == a.numel()
    got, f64, yard = torch.cat(got), torch.cat(f64), torch.cat(yard)
    cpu, err = R.rel_err(yard, f64), R.rel_err(got, f64)
    print('ERR %-44s %-4s %-7s hip %.2e  fp32-cpu %.2e  bar %.0e' % ('valid chain 64->64->128->128', 'pool', FAM, err, cpu, bar))
    assert cpu <= bar / 8, 'input too hard for the bar: fp32 yardstick %.3e, bar %.1e' % (cpu, bar)
    assert err <= bar, 'chain: HIP is %.3e of the max from float64 (bar %.1e, fp32 yardstick on the CPU: %.3e)' % (err, bar, cpu)


def test_valid_height_argument_checks():
    """dgrad = 1, a mask, or null heights: an error code and a message, nothing launched (output and workspace keep their NaN prefill)."""
    lib = _lib()
    so = lib.load()
    x, w, b = torch.zeros(1, 8, 8, 64, device=DEV), torch.zeros(64, 64, 3, 3, device=DEV), torch.zeros(64, device=DEV)
    valid = torch.tensor([8], dtype=torch.int32).to(DEV)
    out = _Out((1, 8, 8, 64))
    ws, wsb = _ws(lib.query('re2e_conv3x3_wino_workspace_bytes', 64, 64))
    for what, dgrad, mask, vr in (('dgrad', 1, None, valid), ('mask', 0, x, valid), ('null heights', 0, None, None)):
        rc = so.re2e_conv3x3_wino_valid(x.data_ptr(), 1, 8, 8, 64, w.data_ptr(), 64, dgrad, b.data_ptr(), 1, None if mask is None else mask.data_ptr(),
                                        out.ptr(), None, None, None if vr is None else vr.data_ptr(), ws.data_ptr(), wsb, lib.stream())
        assert rc != 0, what
        assert len(so.re2e_last_error()) > 0, what
    assert torch.isnan(_guarded(out, 'argument checks')).all() and torch.isnan(ws.cpu()).all(), 'a refused call launched something'
    with pytest.raises(lib.Re2eError):
        lib.call('re2e_conv3x3_wino_valid', x.data_ptr(), 1, 8, 8, 64, w.data_ptr(), 64, 1, b.data_ptr(), 1, None, out.ptr(), None, None, valid.data_ptr(),
                 ws.data_ptr(), wsb)
