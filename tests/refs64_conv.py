"""Float64 reference of the convolutions at their C-ABI contract (csrc/igemm.hip, gemm_nt.hip, conv3x3.hip, thinconv.hip, winograd.hip,
wino_wgrad.hip, wino44.hip) and the inputs of tests/test_conv_kernels_gpu.py.

Plain torch on the CPU, nothing imported from the product or from ``oracle``.  The layer reference is written out tap by tap over NHWC
tensors (one matrix product per tap, no F.conv2d, no autograd), so that it is a second derivation and so that the deliberate ``MISTAKES``
have a place to go; tests/test_refs64_conv_cpu.py pins it to F.conv2d / F.conv_transpose2d / autograd / F.max_pool2d on doubles.  Like the
references of tests/refs64.py it takes ``dtype``: float64 is the yardstick, the SAME code in float32 says how far fp32 arithmetic alone is
from it on a given input.  For the Winograd families that fp32 yardstick is an evaluation of the Winograd algorithms themselves
(``wino_fwd`` / ``wino_wgrad``, F(2x2,3x3) and F(2x2,4x4), matrices below); the float64 truth stays the direct convolution.

``CONV_CASES`` holds one row per kernel form the plans (re2e_conv_plan: csrc/igemm.hip plan_conv_layer / plan_conv) can name on a 256-CU
chip, keyed by ``form_key``, plus the sub-forms the Winograd files branch on below the plan (``sub``); tests/test_refs64_conv_cpu.py
checks that the table is closed under a sweep of the plans.

Every input here is finite.  What the same forms make of a NaN or an infinity in x or dz is tests/refs64_nonfinite.py's subject (poison_conv).
"""
import collections

import torch
import torch.nn.functional as F

from refs64 import rel_err, rnd          # noqa: F401  (re-exported: the convolution tests use them through this module)

# ---------------------------------------------------------------------------------------------
# The bars: 8 x the worst distance of the fp32 CPU yardstick from float64 over every row of CONV_CASES, rounded up to one significant
# digit (tests/test_refs64_conv_cpu.py recomputes the measured values and asserts every row within an eighth of its bar; no bar may
# exceed BAR_CAP).  Key: (quantity, family); measured worst value beside each.
# ---------------------------------------------------------------------------------------------
BAR_CAP = 5e-5
BARS = {
    ('y', 'direct'): 2e-6,           # 1.95e-7
    ('dx', 'direct'): 2e-6,          # 2.03e-7
    ('dW', 'direct'): 4e-6,          # 4.53e-7  (3 x 37 x 20 pixels, 1 -> 8 channels, through the ReLU)
    ('db', 'direct'): 9e-7,          # 1.12e-7  (the column sum beside every family's weight gradient; over LAYERS)
    ('pool', 'direct'): 2e-6,        # 1.44e-7
    ('y', 'wino3x3'): 2e-6,          # 2.05e-7
    ('dx', 'wino3x3'): 2e-6,         # 2.01e-7
    ('dW', 'wino3x3'): 5e-6,         # 5.51e-7  (3 x 64 x 64 pixels)
    ('pool', 'wino3x3'): 3e-6,       # 2.97e-7
    ('y', 'wino4x4'): 8e-6,          # 9.21e-7  (F(2x2,4x4) amplifies: its B^T rows sum to 6 in absolute value, F(2x2,3x3)'s to 2)
    ('dx', 'wino4x4'): 1e-5,         # 1.13e-6
    ('dW', 'wino4x4'): 3e-5,         # 3.38e-6  (2 x 67 x 67 pixels, 64 -> 128 channels)
}

# deliberate mistakes the sensitivity test applies to the reference (never used for a yardstick)
MISTAKES = {
    'a': 'the last image column of one channel read as padding',
    'b': 'two parity classes of the stride-2 data gradient exchanged',
    'c': 'the last 16 pixels left out of the weight gradient\'s pixel sum',
    'd': 'the ReLU mask taken as >= 0',
    'e': 'the odd last row of the ceil-mode pool dropped',
    'f': 'beta ignored',
    'g': 'both operands rounded to 11 mantissa bits',
}

FWD, DGRAD, WGRAD = 0, 1, 2          # re2e_conv_plan's directions
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 2, 3          # include/re2e.h RE2E_ACT_*
F_BIAS, F_POOL, F_MASK, F_W_STRIDED, F_X_STRIDED, F_DZ_STRIDED, F_NO_WINO, F_NO_WINO_WGRAD, F_UNALIGNED, F_FILLER = (1 << i for i in range(10))
F_DIRECT = F_NO_WINO | F_NO_WINO_WGRAD


def round11(t):
    """Every element rounded to 11 mantissa bits behind the leading one (mistake 'g': what a product on a reduced-precision matrix path would see)."""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 4096.0) / 4096.0, e).to(t.dtype)


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def _pad_hw(x, p):
    return F.pad(x, (0, 0, p, p, p, p))


def _act(v, act):
    if act == ACT_RELU:
        return torch.clamp(v, min=0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    assert act == ACT_NONE
    return v


SUM_BLOCK = 32          # terms per block of a float32 sum


def _mm(a, b):
    """a (P,C) @ b (C,K).  float64: torch's own product (its rounding, 1e-16, is nine orders under every bar).  float32: the sum over C written
    out with elementwise operations alone -- blocks of SUM_BLOCK terms summed pairwise, the blocks accumulated in sequence, which is the order of
    a tiled kernel -- so that the fp32 yardstick is the same number on every machine, whatever BLAS, thread count or vector width it has."""
    if a.dtype != torch.float32:
        return a @ b
    P, C = a.shape
    K = b.shape[1]
    step = max(1, (1 << 22) // (SUM_BLOCK * K))
    if P > step:
        return torch.cat([_mm(a[i:i + step], b) for i in range(0, P, step)])
    acc = torch.zeros(P, K, dtype=a.dtype)
    for c0 in range(0, C, SUM_BLOCK):
        t = a[:, c0:c0 + SUM_BLOCK, None] * b[None, c0:c0 + SUM_BLOCK, :]
        if t.shape[1] < SUM_BLOCK:
            t = F.pad(t, (0, 0, 0, SUM_BLOCK - t.shape[1]))          # adding zeros is exact
        n = SUM_BLOCK
        while n > 1:
            n //= 2
            t = t[:, :n] + t[:, n:2 * n]
        acc += t[:, 0]
    return acc


def _lin(M, t, dim):
    """A small constant matrix M (rows of Python floats) applied along ``dim`` of t, term by term (no BLAS: see _mm)."""
    parts = t.unbind(dim)
    rows = []
    for coef in M:
        acc = None
        for c, part in zip(coef, parts):
            if c != 0:
                acc = part * c if acc is None else acc + part * c
        rows.append(acc if acc is not None else torch.zeros_like(parts[0]))
    return torch.stack(rows, dim)


# ---------------------------------------------------------------------------------------------
# the layer, tap by tap.  x (N,H,W,Cin), w (Cout,Cin,KH,KW) as nn.Conv2d stores it, dz (N,OH,OW,Cout)
# ---------------------------------------------------------------------------------------------
def conv_fwd(x, w, b=None, stride=1, pad=1, act=ACT_NONE, y0=None, dtype=torch.float64, mistake=None):
    """act(conv(x, w) + b) (+ y0: the beta = 1 accumulation, added AFTER the activation as the kernels' epilogue does) -> (N,OH,OW,Cout)."""
    x, w = x.to(dtype), w.to(dtype)
    if mistake == 'a':
        x = x.clone()
        x[:, :, -1, 0] = 0
    if mistake == 'g':
        x, w = round11(x), round11(w)
    N, H, W, C = x.shape
    K, _, KH, KW = w.shape
    OH, OW = conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad)
    xp = _pad_hw(x, pad)
    y = torch.zeros(N, OH, OW, K, dtype=dtype)
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :]
            y += _mm(xs.reshape(-1, C), w[:, :, kh, kw].t().contiguous()).view(N, OH, OW, K)
    if b is not None:
        y = y + b.to(dtype)
    y = _act(y, act)
    if y0 is not None and mistake != 'f':
        y = y + y0.to(dtype)
    return y


def conv_dgrad(dz, w, H, W, stride=1, pad=1, relu_out=None, dtype=torch.float64, mistake=None):
    """d sum(conv(x, w) * dz) / dx -> (N,H,W,Cin): stride 1, or stride 2 with even kernels (the four output parity classes);
    ``relu_out``: x was the ReLU output of the layer in front, the gradient passes only where it is > 0 (exact zeros block)."""
    dz, w = dz.to(dtype), w.to(dtype)
    if mistake == 'a':
        dz = dz.clone()
        dz[:, :, -1, 0] = 0
    if mistake == 'g':
        dz, w = round11(dz), round11(w)
    N, OH, OW, K = dz.shape
    _, C, KH, KW = w.shape
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=dtype)
    for kh in range(KH):
        for kw in range(KW):
            dxp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :] += _mm(dz.reshape(-1, K), w[:, :, kh, kw].contiguous()).view(N, OH, OW, C)
    dx = dxp[:, pad:pad + H, pad:pad + W, :].clone()
    if mistake == 'b':
        assert stride == 2
        a, b = dx[:, 0::2, 1::2].clone(), dx[:, 1::2, 0::2].clone()          # classes (0, 1) and (1, 0), over the part both have
        h, w = min(a.shape[1], b.shape[1]), min(a.shape[2], b.shape[2])
        dx[:, 0:2 * h:2, 1:2 * w:2], dx[:, 1:2 * h:2, 0:2 * w:2] = b[:, :h, :w], a[:, :h, :w]
    if relu_out is not None:
        keep = relu_out.to(dtype) >= 0 if mistake == 'd' else relu_out.to(dtype) > 0
        dx = torch.where(keep, dx, torch.zeros_like(dx))
    return dx


def conv_wgrad(x, dz, KH, KW, stride=1, pad=1, dW0=None, dtype=torch.float64, mistake=None):
    """d sum(conv(x, w) * dz) / dw (+ dW0: beta = 1) -> (Cout,Cin,KH,KW).  The pixel sum runs image by image: what the float32 run of it
    measures is then the sum of a split-K kernel: slices of the pixel axis, added at the end."""
    x, dz = x.to(dtype), dz.to(dtype)
    if mistake == 'a':
        x = x.clone()
        x[:, :, -1, 0] = 0
    if mistake == 'c':
        dz = dz.clone()
        dz.view(-1, dz.shape[3])[-16:] = 0
    if mistake == 'g':
        x, dz = round11(x), round11(dz)
    N, OH, OW, K = dz.shape
    C = x.shape[3]
    xp = _pad_hw(x, pad)
    dW = torch.zeros(K, C, KH, KW, dtype=dtype)
    for n in range(N):
        d2 = dz[n].reshape(-1, K).t()
        for kh in range(KH):
            for kw in range(KW):
                xs = xp[n, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :]
                dW[:, :, kh, kw] += _mm(d2, xs.reshape(-1, C))
    if dW0 is not None and mistake != 'f':
        dW = dW + dW0.to(dtype)
    return dW


def bias_grad(dz, dtype=torch.float64):
    d2 = dz.to(dtype).reshape(-1, dz.shape[-1])
    return _mm(d2.t().contiguous(), torch.ones(d2.shape[0], 1, dtype=dtype))[:, 0]


def conv_transpose_fwd(x, wt, b=None, pad=1, dtype=torch.float64, mistake=None):
    """nn.ConvTranspose2d(C1, C2, 2 pad + 2, stride 2, padding pad) over NHWC: x (N,H,W,C1), wt (C1,C2,KH,KW) -> (N,2H,2W,C2).  It IS the data
    gradient of the stride-2 convolution with that weight."""
    N, H, W, _ = x.shape
    y = conv_dgrad(x, wt, 2 * H, 2 * W, 2, pad, dtype=dtype, mistake=mistake)
    return y if b is None else y + b.to(dtype)


def conv_transpose_grads(x, wt, dy, pad=1, dtype=torch.float64, mistake=None):
    """-> (dx, dwt, db) of sum(conv_transpose_fwd(x, wt, b) * dy): a stride-2 forward convolution of dy, and the weight gradient with the
    roles of input and output gradient exchanged."""
    KH, KW = wt.shape[2], wt.shape[3]
    return (conv_fwd(dy, wt, None, 2, pad, dtype=dtype, mistake=mistake), conv_wgrad(dy, x, KH, KW, 2, pad, dtype=dtype, mistake=mistake),
            bias_grad(dy, dtype))


def relu_pool(y, mistake=None):
    """2x2 / stride-2 ceil-mode max pool of a ReLU output y (N,H,W,C) -> (values (N,ceil(H/2),ceil(W/2),C), index bytes uint8) by the rule
    re2e_maxpool2_fwd documents for relu_in = 1: the index is dy * 2 + dx of the FIRST maximum of the window in row-major order (positions
    outside the image never win), and 4 where that maximum is not > 0 (the whole window is ReLU zeros: nothing passes back)."""
    N, H, W, C = y.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    yp = F.pad(y, (0, 0, 0, 2 * OW - W, 0, 2 * OH - H), value=float('-inf'))
    win = yp.view(N, OH, 2, OW, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, OH, OW, C, 4)
    best = win.max(dim=4).values
    idx = torch.full(best.shape, 3, dtype=torch.uint8)
    for d in (2, 1, 0):
        idx = torch.where(win[..., d] == best, torch.full_like(idx, d), idx)
    idx = torch.where(best > 0, idx, torch.full_like(idx, 4))
    if mistake == 'e':
        assert H % 2 == 1
        best, idx = best.clone(), idx.clone()
        best[:, -1] = 0
        idx[:, -1] = 4
    return best, idx


# ---------------------------------------------------------------------------------------------
# The Winograd algorithms themselves: Y = A^T [ (G g G^T) . (B^T d B) ] A over 2x2 output tiles.  F(2x2,3x3): the matrices of Lavin & Gray
# (winograd.hip, wino_wgrad.hip); F(2x2,4x4): interpolation points (0, 1, -1, 2, inf) as wino44.hip states them.
# ---------------------------------------------------------------------------------------------
WINO = {
    3: dict(BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
            G=[[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
            AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: dict(BT=[[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]],
            G=[[.5, 0, 0, 0], [-.5, -.5, -.5, -.5], [-1 / 6, 1 / 6, -1 / 6, 1 / 6], [1 / 6, 1 / 3, 2 / 3, 4 / 3], [0, 0, 0, 1]],
            AT=[[1, 1, 1, 1, 0], [0, 1, -1, 2, 1]]),
}


def _t2(M, t):
    """M t M^T over the last two axes of t."""
    return _lin(M, _lin(M, t, t.dim() - 2), t.dim() - 1)


def _tr(M):
    return [list(col) for col in zip(*M)]


def _wino_tiles(x, r, pad, ty, tx):
    """(N,ty,tx,C,a,a): the (r + 1)^2 input patch of every 2x2 output tile, zero outside the image."""
    N, H, W, C = x.shape
    a = r + 1
    xp = F.pad(x, (0, 0, pad, 2 * tx + r - 1 - W - pad, pad, 2 * ty + r - 1 - H - pad))
    return xp.unfold(1, a, 2).unfold(2, a, 2)


def wino_fwd(x, w, pad, dtype=torch.float32):
    """conv(x, w), stride 1, by F(2x2,rxr) in ``dtype``: x (N,H,W,C), w (K,C,r,r) -> (N,OH,OW,K)."""
    x, w = x.to(dtype), w.to(dtype)
    r, m = w.shape[2], WINO[w.shape[2]]
    N, H, W, C = x.shape
    K = w.shape[0]
    OH, OW = H + 2 * pad - r + 1, W + 2 * pad - r + 1
    ty, tx = (OH + 1) // 2, (OW + 1) // 2
    V = _t2(m['BT'], _wino_tiles(x, r, pad, ty, tx)).reshape(N * ty * tx, C, r + 1, r + 1)
    U = _t2(m['G'], w)                                                                        # (K,C,a,a)
    M = torch.stack([torch.stack([_mm(V[:, :, i, j].contiguous(), U[:, :, i, j].t().contiguous()) for j in range(r + 1)], 2) for i in range(r + 1)], 2)
    Y = _t2(m['AT'], M).view(N, ty, tx, K, 2, 2)
    return Y.permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * ty, 2 * tx, K)[:, :OH, :OW].contiguous()


def wino_dgrad(dz, w, pad, dtype=torch.float32):
    """The stride-1 data gradient the same way: a forward of dz with the weights rotated by 180 degrees and their channel axes exchanged."""
    r = w.shape[2]
    return wino_fwd(dz, w.flip(2, 3).transpose(0, 1), r - 1 - pad, dtype)


def wino_wgrad(x, dz, r, pad, dtype=torch.float32):
    """dW = G^T [ sum over tiles of (B^T d B) (x) (A dY A^T) ] G -> (K,C,r,r)."""
    x, dz = x.to(dtype), dz.to(dtype)
    m = WINO[r]
    N, OH, OW, K = dz.shape
    C = x.shape[3]
    ty, tx = (OH + 1) // 2, (OW + 1) // 2
    V = _t2(m['BT'], _wino_tiles(x, r, pad, ty, tx)).reshape(N * ty * tx, C, r + 1, r + 1)                # (tiles,C,a,a)
    dy = F.pad(dz, (0, 0, 0, 2 * tx - OW, 0, 2 * ty - OH)).view(N, ty, 2, tx, 2, K).permute(0, 1, 3, 5, 2, 4)
    Mdy = _t2(_tr(m['AT']), dy).reshape(N * ty * tx, K, r + 1, r + 1)                                     # (tiles,K,a,a)
    S = torch.stack([torch.stack([_mm(Mdy[:, :, i, j].t().contiguous(), V[:, :, i, j].contiguous()) for j in range(r + 1)], 2) for i in range(r + 1)], 2)
    return _t2(_tr(m['G']), S)


# ---------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------
def form_key(direction, p):
    """The kernel form a re2e_conv_plan answer (a dict of strings) names, as CONV_CASES writes it."""
    if p['family'] != 'direct':
        return (p['family'], direction)
    r = p['route']
    if r == 'engine':
        return (r, direction, p['tile'], int(p['vec']), int(p['mask_pass']))
    if r == 'pipeline':
        return (r, direction, int(p['variant']), p['tile'])
    if r == 'cout1':
        return (r, direction, int(p['L']), int(p['kh']), int(p['kw']), int(p['ch']))
    if r == 'cin1_fwd':
        return (r, direction, p['taps'])
    if r == 'halo':
        return (r, direction, p['patch'], int(p['dir']), int(p['relu']), int(p['fused_pool']))
    if r == 'wgrad_engine':
        return (r, p['tile'], int(p['vec']), int(p['wide_reduce']), int(int(p['splits']) > 1))
    if r in ('wgrad_cin1', 'wgrad_cout1'):
        return (r, int(p['wide_reduce']), int(int(p['slabs']) > 1))
    return (r, direction)


Row = collections.namedtuple('Row', 'form direction N H W Cin Cout k stride pad act flags beta sub via')


def _row(form, direction, N, H, W, Cin, Cout, k, stride=1, act=ACT_NONE, flags=0, beta=0, sub=None, via=None):
    """form: the plan's form_key (None, edges: whatever the plan names); sub: the sub-form below the plan; via: the family whose entry point the
    row calls where that is not the family the layer plan names ('wino3x3' / 'wino4x4': shapes the entry points take and the plan never sends)."""
    return Row(form, direction, N, H, W, Cin, Cout, k, stride, 1, act, flags, beta, sub, via)


def plan_args(row):
    """The arguments of lib.conv_plan for a row (cus aside)."""
    return (row.direction, row.N, row.H, row.W, row.Cin, row.Cout, row.k, row.k, row.stride, row.pad, 0, 0, row.act), row.flags


_E, _P, _H, _C1, _WE = 'engine', 'pipeline', 'halo', 'cout1', 'wgrad_engine'
_HB = F_BIAS | F_POOL | F_NO_WINO
CONV_CASES = (
    # ---- thin kernels (thinconv.hip): Cin == 1 forward both tap counts, as the data gradient of a Cout == 1 layer too
    [_row(('cin1_fwd', FWD, '3x3'), FWD, 1, 5, 3, 1, 4, 3), _row(('cin1_fwd', FWD, '4x4'), FWD, 1, 5, 3, 1, 4, 4),
     _row(('cin1_fwd', DGRAD, '3x3'), DGRAD, 1, 5, 3, 4, 1, 3), _row(('cin1_fwd', DGRAD, '4x4'), DGRAD, 1, 5, 3, 4, 1, 4)] +
    # the generic cout1<L,0,0,0> at every L, forward (Cin = 4 L) and as the data gradient of a Cin == 1 layer (Cout = 4 L)
    [_row((_C1, FWD, L, 0, 0, 0), FWD, 2, 5, 7, 4 * L, 1, 3) for L in (1, 2, 4, 8, 32, 64)] +
    [_row((_C1, FWD, 16, 0, 0, 0), FWD, 2, 5, 7, 64, 1, 4)] +
    [_row((_C1, DGRAD, L, 0, 0, 0), DGRAD, 2, 5, 7, 1, 4 * L, 3) for L in (1, 2, 4, 8, 32, 64)] +
    [_row((_C1, DGRAD, 16, 0, 0, 0), DGRAD, 2, 5, 7, 1, 64, 4)] +
    # the compile-time tap counts of the training step
    [_row((_C1, FWD, 16, 3, 3, 1), FWD, 1, 5, 3, 64, 1, 3), _row((_C1, FWD, 64, 4, 4, 2), FWD, 1, 5, 3, 512, 1, 4),
     _row((_C1, DGRAD, 16, 3, 3, 1), DGRAD, 1, 5, 3, 1, 64, 3), _row((_C1, DGRAD, 16, 2, 2, 1), DGRAD, 1, 6, 4, 1, 64, 4, stride=2),
     _row((_C1, DGRAD, 64, 4, 4, 2), DGRAD, 1, 5, 3, 1, 512, 4),
     _row(('cout1_rows', FWD), FWD, 1, 35, 19, 64, 1, 3), _row(('cout1_rows', DGRAD), DGRAD, 1, 35, 19, 1, 64, 3)] +
    # ---- the engine (igemm.hip): every tile x 16-byte loads or not x the separate mask pass
    [_row((_E, FWD, '128x128x16', 0, 0), FWD, 1, 5, 3, 1, 96, 3), _row((_E, FWD, '128x128x16', 1, 0), FWD, 1, 5, 3, 4, 96, 3),
     _row((_E, FWD, '256x128x16', 1, 0), FWD, 1, 66, 66, 4, 96, 3),
     _row((_E, FWD, '256x32x32', 0, 0), FWD, 1, 5, 3, 1, 1, 3, flags=F_UNALIGNED), _row((_E, FWD, '256x32x32', 1, 0), FWD, 1, 5, 3, 4, 2, 3),
     _row((_E, FWD, '256x64x16', 0, 0), FWD, 1, 5, 3, 1, 36, 3), _row((_E, FWD, '256x64x16', 1, 0), FWD, 1, 5, 3, 4, 36, 3),
     _row((_E, DGRAD, '128x128x16', 0, 0), DGRAD, 1, 5, 3, 96, 1, 3), _row((_E, DGRAD, '128x128x16', 0, 1), DGRAD, 1, 5, 3, 96, 1, 3, flags=F_MASK),
     _row((_E, DGRAD, '128x128x16', 1, 0), DGRAD, 1, 5, 3, 96, 4, 3), _row((_E, DGRAD, '128x128x16', 1, 1), DGRAD, 1, 5, 3, 96, 4, 3, flags=F_MASK),
     _row((_E, DGRAD, '256x128x16', 1, 0), DGRAD, 1, 66, 66, 96, 4, 3), _row((_E, DGRAD, '256x128x16', 1, 1), DGRAD, 1, 66, 66, 96, 4, 3, flags=F_MASK),
     _row((_E, DGRAD, '256x32x32', 0, 0), DGRAD, 1, 5, 3, 1, 1, 3, flags=F_UNALIGNED),
     _row((_E, DGRAD, '256x32x32', 0, 1), DGRAD, 1, 5, 3, 1, 1, 3, flags=F_MASK | F_UNALIGNED),
     _row((_E, DGRAD, '256x32x32', 1, 0), DGRAD, 1, 5, 3, 3, 4, 3), _row((_E, DGRAD, '256x32x32', 1, 1), DGRAD, 1, 5, 3, 1, 4, 3, flags=F_MASK),
     _row((_E, DGRAD, '256x64x16', 0, 0), DGRAD, 1, 5, 3, 36, 1, 3), _row((_E, DGRAD, '256x64x16', 0, 1), DGRAD, 1, 5, 3, 36, 1, 3, flags=F_MASK),
     _row((_E, DGRAD, '256x64x16', 1, 0), DGRAD, 1, 5, 3, 36, 4, 3), _row((_E, DGRAD, '256x64x16', 1, 1), DGRAD, 1, 5, 3, 36, 4, 3, flags=F_MASK)] +
    # ---- the halo-patch kernel (conv3x3.hip): both patches x no ReLU / ReLU / ReLU + fused pool, and as a plain data gradient
    [_row((_H, FWD, '16x16', 1, 0, 0), FWD, 1, 5, 3, 16, 64, 3, flags=F_DIRECT), _row((_H, FWD, '16x16', 1, 1, 0), FWD, 1, 5, 3, 16, 64, 3, act=ACT_RELU, flags=F_DIRECT),
     _row((_H, FWD, '16x16', 1, 1, 1), FWD, 1, 5, 3, 16, 64, 3, act=ACT_RELU, flags=_HB),
     _row((_H, FWD, '32x8', 1, 0, 0), FWD, 2, 33, 8, 16, 64, 3, flags=F_DIRECT), _row((_H, FWD, '32x8', 1, 1, 0), FWD, 2, 33, 8, 16, 64, 3, act=ACT_RELU, flags=F_DIRECT),
     _row((_H, FWD, '32x8', 1, 1, 1), FWD, 2, 33, 8, 16, 64, 3, act=ACT_RELU, flags=_HB),
     _row((_H, DGRAD, '16x16', -1, 0, 0), DGRAD, 1, 5, 3, 64, 16, 3, flags=F_DIRECT), _row((_H, DGRAD, '32x8', -1, 0, 0), DGRAD, 2, 33, 8, 64, 16, 3, flags=F_DIRECT)] +
    # ---- the pipeline (gemm_nt.hip) under a convolution: the largest tensors of the table (variant 3: 16 x 64 x 64 x 96, 25 MB)
    [_row((_P, FWD, 3, '256x128x16'), FWD, 16, 64, 64, 16, 96, 3), _row((_P, FWD, 6, '128x128x16'), FWD, 8, 64, 40, 16, 96, 3),
     _row((_P, FWD, 8, '128x64x16'), FWD, 2, 33, 8, 16, 4, 3),
     _row((_P, DGRAD, 3, '256x128x16'), DGRAD, 16, 64, 64, 96, 16, 3), _row((_P, DGRAD, 6, '128x128x16'), DGRAD, 8, 64, 40, 96, 16, 3),
     _row((_P, DGRAD, 8, '128x64x16'), DGRAD, 2, 33, 8, 4, 16, 3)] +
    # ---- weight gradients: the thin kernels with one slab, several, and the wide reduce; the engine's tiles x 16-byte loads x reduce x slabs
    [_row(('wgrad_cin1', 0, 0), WGRAD, 1, 5, 3, 1, 4, 3), _row(('wgrad_cin1', 0, 1), WGRAD, 1, 9, 8, 1, 4, 3), _row(('wgrad_cin1', 1, 1), WGRAD, 8, 64, 40, 1, 4, 3),
     _row(('wgrad_cout1', 0, 0), WGRAD, 1, 5, 3, 4, 1, 3), _row(('wgrad_cout1', 0, 1), WGRAD, 2, 33, 8, 4, 1, 3), _row(('wgrad_cout1', 1, 1), WGRAD, 2, 64, 64, 4, 1, 3)] +
    [_row((_WE, tile, vec, wr, sp), WGRAD, *shape, Cin if vec else 1, Cout if vec else Cout0, 3)
     for tile, Cin, Cout, Cout0 in (('128x128x16', 4, 96, 96), ('256x32x32', 4, 4, 1), ('256x64x16', 4, 36, 36))
     for vec in (0, 1) for wr, sp, shape in ((0, 0, (1, 5, 3)), (0, 1, (2, 33, 8)), (1, 1, (8, 64, 40)))] +
    [_row((_WE, '192x64x16', 1, 0, 0), WGRAD, 1, 5, 3, 12, 36, 4), _row((_WE, '192x64x16', 1, 0, 1), WGRAD, 1, 35, 19, 12, 36, 4),
     _row((_WE, '192x64x16', 1, 1, 1), WGRAD, 8, 64, 40, 12, 36, 4)] +
    # ---- Winograd F(2x2,3x3) (winograd.hip): the plan's three forms, then both patch shapes x {C = 64 staged, C % 64 staged in passes,
    # per-lane loads} x 1, 2, 4 channel groups
    [_row(('wino3x3', FWD), FWD, 1, 5, 3, 8, 64, 3, sub=('wide', 'lanes', 1)), _row(('wino3x3', DGRAD), DGRAD, 1, 5, 3, 64, 8, 3, sub=('wide', 'lanes', 1)),
     _row(('wino3x3', DGRAD), DGRAD, 1, 30, 7, 64, 128, 3, flags=F_MASK, sub=('tall', 'passes', 1))] +
    [_row(('wino3x3', FWD), FWD, 1, H, W, C, 64 * g, 3, act=ACT_RELU if g == 2 else ACT_NONE, flags=F_BIAS if g != 4 else 0, sub=(shape, cname, g))
     for shape, H, W in (('wide', 7, 30), ('tall', 30, 7)) for cname, C in (('c64', 64), ('passes', 128), ('lanes', 72)) for g in (1, 2, 4)] +
    [_row(('wino3x3', FWD), FWD, 2, 9, 17, 64, 64, 3, act=ACT_RELU, flags=F_BIAS | F_POOL, sub=('tall', 'c64', 1))] +
    # wino_wgrad.hip: both patch shapes; one patch range, a number that is no multiple of 8 (idle workgroups), 8 and 12; beta 0 / 1
    [_row(('wino3x3', WGRAD), WGRAD, 1, 30, 7, 64, 64, 3, sub=('tall', 1)), _row(('wino3x3', WGRAD), WGRAD, 2, 40, 48, 64, 128, 3, beta=1, sub=('wide', 3)),
     _row(('wino3x3', WGRAD), WGRAD, 2, 64, 24, 128, 64, 3, sub=('tall', 3)), _row(('wino3x3', WGRAD), WGRAD, 2, 64, 64, 64, 64, 3, beta=1, sub=('wide', 8)),
     _row(('wino3x3', WGRAD), WGRAD, 3, 64, 64, 64, 64, 3, sub=('wide', 12))] +
    # ---- Winograd F(2x2,4x4) (wino44.hip): forward (pad 1), data gradient (pad 2), weight gradient with one K slice per position and with
    # two over zero-padded tiles (sub = 2, Ppad > P)
    [_row(('wino4x4', FWD), FWD, 1, 65, 65, 64, 64, 4), _row(('wino4x4', DGRAD), DGRAD, 1, 66, 66, 64, 64, 4),
     _row(('wino4x4', WGRAD), WGRAD, 1, 65, 65, 64, 64, 4, beta=1, sub=('sub', 1, 'exact')),
     _row(('wino4x4', WGRAD), WGRAD, 2, 67, 67, 64, 128, 4, sub=('sub', 2, 'padded'))])


# ---------------------------------------------------------------------------------------------
# Edges the table does not turn (form None: the row runs whatever the plan names and prints it).  Sizes of 1 and 2; one below / at / one above
# the patch and tile edges (8, 16, 32 rows or columns; the 16-row tiles of cout1_rows; 2x2 output tiles with odd OH, OW); channel counts at
# both sides of every eligibility predicate; beta = 1 on every route that has it; stride 2; unaligned operands (views 4 bytes into a larger
# allocation) and a filler stream; the widths at which cout1_rows' table stops fitting a CU's LDS; Cout of 32, 96, 192 on the Winograd
# weight gradient, which its entry point takes and the layer plan never sends.
# ---------------------------------------------------------------------------------------------
def _three(N, H, W, Cin, Cout, k=3, stride=1, **kw):
    return [_row(None, d, N, H, W, Cin, Cout, k, stride, **kw) for d in (FWD, DGRAD, WGRAD)]


_CHANNELS = ((3, 10), (4, 10), (5, 10), (8, 64), (12, 64), (16, 64), (24, 64), (16, 32), (16, 36), (16, 68), (64, 128), (64, 192), (64, 256))
EDGES = (
    [r for shape in ((1, 1, 7), (1, 7, 1), (2, 2, 2), (1, 1, 1)) for cin, cout in ((6, 10), (64, 64), (1, 8), (8, 1)) for r in _three(*shape, cin, cout)] +
    [r for shape in ((1, 1, 7), (2, 2, 2)) for r in _three(*shape, 16, 64, flags=F_DIRECT)] +
    # halo patches: 16x16 and 32x8
    [_row(None, d, 1, H, W, 16, 64, 3, flags=F_DIRECT) for d in (FWD, DGRAD) for H, W in ((15, 17), (16, 16), (17, 15), (31, 8), (32, 8), (33, 7))] +
    # Winograd F(2x2,3x3) patches: 8 x 16 and 16 x 8 pixels
    [r for H, W in ((7, 17), (8, 16), (9, 15), (15, 9), (16, 8), (17, 7)) for r in _three(1, H, W, 64, 64)] +
    # the row-tile Cout == 1 kernel: 16 rows per workgroup, the narrowest width it takes, a ragged last tile at the widest (250), and the
    # widths above it on cout1<16,3,3,1>
    [_row(None, FWD, 1, H, 20, 64, 1, 3, flags=F_BIAS) for H in (15, 16, 17)] +
    [_row(('cout1_rows', FWD), FWD, 1, 1, 16, 64, 1, 3), _row(('cout1', FWD, 16, 3, 3, 1), FWD, 1, 3, 15, 64, 1, 3),
     _row(('cout1_rows', FWD), FWD, 1, 17, 250, 64, 1, 3, flags=F_BIAS), _row(('cout1_rows', DGRAD), DGRAD, 1, 17, 250, 1, 64, 3),
     _row(('cout1', FWD, 16, 3, 3, 1), FWD, 1, 17, 251, 64, 1, 3, flags=F_BIAS), _row(('cout1', FWD, 16, 3, 3, 1), FWD, 1, 17, 256, 64, 1, 3),
     _row(('cout1', DGRAD, 16, 3, 3, 1), DGRAD, 1, 17, 256, 1, 64, 3)] +
    # Winograd F(2x2,4x4) through its entry points: odd OH / OW (ragged 2x2 tiles), the smallest maps
    [_row(None, d, 1, H, W, 64, 64, 4, via='wino4x4') for d in (FWD, DGRAD, WGRAD) for H, W in ((4, 4), (5, 6), (6, 5), (2, 9))] +
    [_row(None, d, 2, 9, 10, cin, cout, 4, via='wino4x4') for d in (FWD, DGRAD, WGRAD) for cin, cout in ((128, 64), (64, 192))] +
    # the discriminator's last layer (512 -> 1, 4x4: the longest contraction of the thin kernels) on more than one image
    [r for r in _three(2, 12, 9, 512, 1, 4)] +
    # channel counts at both sides of C % 4, % 8, % 16, % 64, Cout <= 32, <= 64, Cout / 64 a power of two (288 pixels: the pipeline's floor is 256)
    [r for cin, cout in _CHANNELS for r in _three(2, 12, 12, cin, cout)] +
    [r for cin, cout in ((16, 64), (24, 64), (64, 128)) for r in _three(2, 12, 12, cin, cout, flags=F_DIRECT)] +
    # beta = 1: the thin, halo, pipeline and engine forwards; the direct weight gradients
    [_row(None, FWD, 2, 5, 7, 32, 1, 3, beta=1), _row(None, FWD, 1, 17, 20, 64, 1, 3, beta=1), _row(None, FWD, 1, 17, 16, 16, 64, 3, flags=F_DIRECT | F_BIAS, beta=1),
     _row(None, FWD, 2, 12, 12, 16, 96, 3, act=ACT_LRELU, beta=1), _row(None, FWD, 1, 5, 3, 4, 36, 3, flags=F_BIAS, beta=1),
     _row(None, WGRAD, 2, 33, 8, 4, 36, 3, beta=1), _row(None, WGRAD, 1, 9, 8, 1, 4, 3, beta=1), _row(None, WGRAD, 2, 33, 8, 4, 1, 3, beta=1),
     _row(None, WGRAD, 8, 64, 40, 4, 36, 3, beta=1)] +
    # pooled forwards: the fused kernel at even and odd sizes, the unfused pair (re2e_conv_igemm + re2e_maxpool2_fwd), Winograd with two groups
    [_row(None, FWD, 1, H, W, cin, cout, 3, act=ACT_RELU, flags=F_BIAS | F_POOL | f)
     for H, W, cin, cout, f in ((16, 16, 16, 64, F_NO_WINO), (17, 15, 16, 64, F_NO_WINO), (1, 1, 16, 64, F_NO_WINO), (9, 7, 6, 10, 0), (17, 15, 64, 128, 0), (2, 2, 64, 64, 0))] +
    # stride 2 (4x4, pad 1): the forward, the four-class data gradient on the engine and on the pipeline, the per-class thin launches
    [r for shape, cin, cout in (((2, 6, 4), 6, 10), ((3, 18, 40), 8, 16), ((2, 18, 40), 64, 128), ((2, 38, 20), 1, 64), ((3, 38, 80), 1, 8)) for r in _three(*shape, cin, cout, 4, 2)] +
    [_row(None, FWD, 3, 38, 80, 1, 8, 4, 2, act=ACT_LRELU, flags=F_BIAS)] +
    # unaligned operands; a filler stream
    [r for cin, cout in ((8, 20), (16, 96), (64, 64)) for r in _three(2, 12, 12, cin, cout, flags=F_UNALIGNED | F_DIRECT)] +
    [_row(None, FWD, 1, 66, 66, 4, 96, 3, flags=F_FILLER), _row(None, DGRAD, 1, 66, 66, 96, 4, 3, flags=F_FILLER), _row(None, WGRAD, 8, 64, 40, 4, 96, 3, flags=F_FILLER),
     _row(None, FWD, 8, 64, 40, 16, 96, 3, flags=F_FILLER)] +
    # re2e_conv3x3_wino_wgrad at the output widths its entry point takes and the layer plan keeps for the direct kernels
    [_row(None, WGRAD, 1, 30, 7, 64, cout, 3, beta=beta, via='wino3x3') for cout, beta in ((32, 0), (96, 1), (192, 0))])

# Whole layers through ops.conv2d / ops.conv_transpose2d (autograd: y, dx, dW and db in one go): (N, H, W, Cin, Cout, k, stride, act, bias, transposed)
LAYERS = (
    (3, 37, 20, 1, 8, 3, 1, ACT_RELU, True, False),
    (3, 18, 40, 8, 16, 4, 2, ACT_NONE, False, False),
    (2, 16, 12, 64, 64, 3, 1, ACT_RELU, True, False),
    (2, 7, 5, 6, 10, 3, 1, ACT_LRELU, True, False),
    (1, 66, 65, 64, 64, 4, 1, ACT_NONE, False, False),
    (2, 9, 10, 16, 8, 4, 2, ACT_NONE, True, True),
    (2, 5, 3, 3, 5, 4, 2, ACT_NONE, False, True),
)

def layer_id(layer):
    N, H, W, Cin, Cout, k, stride, act, bias, transposed = layer
    return '%s%dx%dx%d-%dto%d-k%ds%d-act%d%s' % ('convT-' if transposed else 'conv-', N, H, W, Cin, Cout, k, stride, act, '-bias' if bias else '')


def layer_case(layer):
    """x (N,H,W,Cin), w as the layer stores it ((Cout,Cin,k,k); transposed: (Cin,Cout,k,k)), b, and the gradient ``go`` of the layer's output."""
    N, H, W, Cin, Cout, k, stride, act, bias, transposed = layer
    g = torch.Generator().manual_seed(N * 1000003 + H * 10007 + W * 101 + Cin * 7 + Cout * 3 + k + stride + 17)
    OH, OW = (2 * H, 2 * W) if transposed else (conv_out(H, k, stride, 1), conv_out(W, k, stride, 1))
    wshape = (Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)
    return dict(x=rnd(g, N, H, W, Cin), w=rnd(g, *wshape, scale=(Cin * k * k) ** -0.5), b=rnd(g, Cout, scale=0.3) if bias else None, go=rnd(g, N, OH, OW, Cout))


def layer_ref(layer, case, dtype=torch.float64):
    """y and the gradients of sum(y * go) with respect to x, w and b (None without a bias), NHWC, as ops.conv2d / ops.conv_transpose2d return them."""
    N, H, W, Cin, Cout, k, stride, act, bias, transposed = layer
    x, w, b, go = case['x'], case['w'], case['b'], case['go'].to(dtype)
    if transposed:
        dx, dW, db = conv_transpose_grads(x, w, go, 1, dtype)
        return dict(y=conv_transpose_fwd(x, w, b, 1, dtype), dx=dx, dW=dW, db=db if bias else None)
    pre = conv_fwd(x, w, b, stride, 1, ACT_NONE, dtype=dtype)
    slope = torch.ones_like(pre) if act == ACT_NONE else torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.0 if act == ACT_RELU else 0.2))
    dz = go * slope
    return dict(y=_act(pre, act), dx=conv_dgrad(dz, w, H, W, stride, 1, dtype=dtype), dW=conv_wgrad(x, dz, k, k, stride, 1, dtype=dtype),
                db=bias_grad(dz, dtype) if bias else None)


# Forms that are built and that no plan names through ops.py on any input (kept out of the closure, with the reason).
NEVER_NAMED = {
    ('halo', DGRAD, '16x16', -1, 1, 0): 'the halo kernel\'s data-gradient form with a ReLU epilogue: re2e_conv_igemm takes an activation in any direction, '
                                        'ops.py asks for none on a data gradient',
    ('halo', DGRAD, '32x8', -1, 1, 0): 'the same on the 32x8 patch',
}


def case_id(row):
    d = ('fwd', 'dgrad', 'wgrad')[row.direction]
    form = 'edge' + ('-' + row.via if row.via else '') if row.form is None else \
        '-'.join(str(v) for v in row.form[:1] + row.form[2 if row.form[0] not in ('wgrad_engine', 'wgrad_cin1', 'wgrad_cout1') else 1:])
    return '%s-%s-%dx%dx%d-%dto%d-k%ds%d%s%s%s' % (d, form, row.N, row.H, row.W, row.Cin, row.Cout, row.k, row.stride, '-f%d' % row.flags if row.flags else '',
                                                '-beta1' if row.beta else '', '-' + '-'.join(str(v) for v in row.sub) if row.sub else '')


def family_of(row, plan_family=None):
    """The family whose entry point a row runs: its ``via``, the family its declared form names, or (edges) the family the plan answered."""
    if row.via:
        return row.via
    if row.form is not None:
        return row.form[0] if row.form[0] in ('wino3x3', 'wino4x4') else 'direct'
    assert plan_family is not None
    return plan_family


def quantity_of(row):
    return ('pool' if row.flags & F_POOL else 'y', 'dx', 'dW')[row.direction]


def conv_case(row):
    """The inputs of a row, a function of its geometry and of whether it masks alone: x (N,H,W,Cin) -- a ReLU output (exact zeros) where the row
    takes its data gradient through that ReLU --, w (Cout,Cin,k,k) ~ N(0, 1/fan-in), b, dz (N,OH,OW,Cout) and the tensors beta = 1 accumulates on."""
    g = torch.Generator().manual_seed(row.N * 1000003 + row.H * 10007 + row.W * 101 + row.Cin * 7 + row.Cout * 3 + row.k + row.stride)
    OH, OW = conv_out(row.H, row.k, row.stride, row.pad), conv_out(row.W, row.k, row.stride, row.pad)
    x = rnd(g, row.N, row.H, row.W, row.Cin)
    w = rnd(g, row.Cout, row.Cin, row.k, row.k, scale=(row.Cin * row.k * row.k) ** -0.5)
    b = rnd(g, row.Cout, scale=0.3)
    dz = rnd(g, row.N, OH, OW, row.Cout)
    y0, dW0 = rnd(g, row.N, OH, OW, row.Cout), rnd(g, row.Cout, row.Cin, row.k, row.k)
    if row.flags & F_MASK:
        x = torch.clamp(x, min=0)
    return dict(x=x, w=w, b=b, dz=dz, y0=y0, dW0=dW0, OH=OH, OW=OW)


def case_ref(row, case, dtype=torch.float64, mistake=None):
    """What the row's entry point is to produce, from the layer reference in ``dtype`` -> tensor (pooled rows: (values, index bytes))."""
    b = case['b'] if row.flags & F_BIAS else None
    if row.direction == FWD:
        y = conv_fwd(case['x'], case['w'], b, row.stride, row.pad, row.act, case['y0'] if row.beta else None, dtype, mistake)
        return relu_pool(y, mistake) if row.flags & F_POOL else y
    if row.direction == DGRAD:
        return conv_dgrad(case['dz'], case['w'], row.H, row.W, row.stride, row.pad, case['x'] if row.flags & F_MASK else None, dtype, mistake)
    return conv_wgrad(case['x'], case['dz'], row.k, row.k, row.stride, row.pad, case['dW0'] if row.beta else None, dtype, mistake)


def case_yardstick(row, case, fam):
    """The fp32 CPU yardstick of a row that runs on family ``fam``: the layer reference in float32, for the Winograd families the fp32 Winograd
    evaluation with the same epilogue (pooled rows: the values)."""
    if fam == 'direct':
        r = case_ref(row, case, torch.float32)
        return r[0] if row.flags & F_POOL else r
    f32 = torch.float32
    if row.direction == FWD:
        y = wino_fwd(case['x'], case['w'], row.pad, f32)
        if row.flags & F_BIAS:
            y = y + case['b']
        y = _act(y, row.act)
        return relu_pool(y)[0] if row.flags & F_POOL else y
    if row.direction == DGRAD:
        dx = wino_dgrad(case['dz'], case['w'], row.pad, f32)
        return torch.where(case['x'] > 0, dx, torch.zeros_like(dx)) if row.flags & F_MASK else dx
    dW = wino_wgrad(case['x'], case['dz'], row.k, row.pad, f32)
    return dW + case['dW0'] if row.beta else dW


def sub_of(row):
    """The sub-form below the plan that a Winograd row reaches, from the arithmetic restated at the end of this file (None: the family has none)."""
    fam = family_of(row)
    if fam == 'wino3x3':
        shape = 'wide' if wino3_wide(row.H, row.W) else 'tall'
        if row.direction == WGRAD:
            return shape, ww_nsplit(row.N, row.H, row.W, row.Cin, row.Cout)
        C, K = (row.Cout, row.Cin) if row.direction == DGRAD else (row.Cin, row.Cout)
        return shape, 'c64' if C == 64 else 'passes' if C % 64 == 0 else 'lanes', K // 64
    if fam == 'wino4x4' and row.direction == WGRAD:
        sub, P, Ppad, _ = w44_wgrad_sub(row.N, row.H, row.W, row.Cin, row.Cout, row.pad)
        return 'sub', sub, 'padded' if Ppad > P else 'exact'
    return None


def mistakes_of(row):
    """The MISTAKES that apply to a row."""
    m = ['a', 'g']
    if row.direction == DGRAD and row.stride == 2:
        m.append('b')
    if row.direction == WGRAD:
        m.append('c')
    if row.flags & F_MASK:
        m.append('d')
    if row.flags & F_POOL and row.H % 2 == 1:
        m.append('e')
    if row.beta:
        m.append('f')
    return sorted(m)


# ---------------------------------------------------------------------------------------------
# the arithmetic of the Winograd files below the plan, restated (tests assert the sub-form a row declares from the libraries' workspace sizes)
# ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def wino3_wide(H, W):
    """winograd.hip / wino_wgrad.hip: 8 x 16 pixel patches (wide) unless 16 x 8 wastes fewer padded pixels."""
    return _cdiv(H, 8) * 8 * _cdiv(W, 16) * 16 <= _cdiv(H, 16) * 16 * _cdiv(W, 8) * 8


def ww_nsplit(N, H, W, C, Cout):
    """wino_wgrad.hip ww_plan: patch ranges per (64 input x 32 output channel) block."""
    wide = wino3_wide(H, W)
    npatch = N * _cdiv(H, 8 if wide else 16) * _cdiv(W, 16 if wide else 8)
    return max(1, min(_cdiv(1536, (C // 64) * (Cout // 32)), npatch // 8))


def ww_workspace_bytes(N, H, W, C, Cout):
    return (ww_nsplit(N, H, W, C, Cout) + 1) * 16 * C * Cout * 4


def w44_wgrad_sub(N, H, W, C, Cout, pad):
    """wino44.hip w44_wgrad_plan -> (K slices per position, tiles P, padded tiles Ppad, workspace bytes)."""
    OH, OW = H + 2 * pad - 3, W + 2 * pad - 3
    P = N * ((OH + 1) // 2) * ((OW + 1) // 2)
    tiles = _cdiv(C, 128) * _cdiv(Cout, 128) * 25
    sub = max(1, min(_cdiv(1024, tiles), P // 1024))
    Ppad = _cdiv(P, 16 * sub) * 16 * sub
    up = lambda v: (v + 255) & ~255
    return sub, P, Ppad, up(25 * Ppad * C * 4) + up(25 * Ppad * Cout * 4) + up(25 * sub * C * Cout * 4)
