"""Float64 references of the feature, normalisation, pooling, loss-reduction and update kernels at their C-ABI contracts -- csrc/fbank.hip
(re2e_fbank_fwd / _bwd, re2e_logclamp_fwd / _bwd, re2e_cmvn_stats) and csrc/elementwise.hip (re2e_bn_lrelu_fwd / _bwd, re2e_bn_apply,
re2e_bn_sync_*, re2e_maxpool2_*, re2e_vgg_pack_*, re2e_loss_fwd / _bwd, re2e_sumsq, re2e_clip_coef, re2e_adadelta_step, re2e_adam_step) --
and the inputs of tests/test_feat_kernels_gpu.py.

Plain torch on the CPU, autograd for the gradients of the filterbank and of BatchNorm (the loss gradients and the pool / pack backward
are the closed forms the ABI documents, pinned to autograd by tests/test_refs64_feat_cpu.py), nothing imported from the product or from
``oracle``.  Every reference takes ``dtype``: float64 is the yardstick, the SAME code in float32 says how far fp32 arithmetic alone is
from it on a given input (``margin_ok``).  Every reference also takes ``mistake``: None, or the name of a wrong variant (``MISTAKES``)
that tests/test_refs64_feat_cpu.py uses to show that the case tables can see a kernel that makes it.

The case tables hold the smallest shapes that reach each branch of the launchers: the 32-frame / 32-filter / 32-bin tiles and 8-bin /
8-filter iterations of the filterbank pair and its 16-byte path, the scalar / float4 partial and apply kernels of BatchNorm and its
1 .. 512 row chunks, the scalar / float4 pool kernels and the tiled / element-wise pack, the grid cap and the 16-byte path of the
reductions, more than one grid sweep of the update kernels.
"""
import math
import os

import numpy as np
import torch

from refs64 import margin_ok, rel_err, rnd          # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAN, INF = float('nan'), float('inf')
CLAMP = 1e-7                # feat_model.py:130 `out[out <= 1e-7] = 1e-7`

# the project's own bars (tests/test_kernels_gpu.py: test_fbank, test_bn_lrelu, test_mean_loss), of the tensor's max
BAR_FBANK_OUT = 1e-5        # y_raw, y_norm, pw_out; the element-wise tail of the dense path; the CMVN sums
BAR_FBANK_GRAD = 1e-4       # dx
BAR_BN_OUT = 1e-5           # y, save_mean, save_invstd, running_mean, running_var
BAR_BN_GRAD = 1e-4          # dx, dgamma, dbeta
BAR_LOSS = 1e-5             # loss values and gradients
BAR_SUM = 1e-6              # re2e_sumsq, the optimizer state tensors, p from step 2 on: a handful of fp32 roundings (6e-8 each) times four,
                            # as for re2e_sgd_step (tests/test_lmseq_kernels_gpu.py)
# p after step 1 from p = 0 (the negated update, read without cancellation): 4 x the worst distance of the fp32 CPU run of adam_ref /
# adadelta_ref from float64 over UPDATE_CASES, rounded up to one significant digit.  That distance depends a little on the CPU (how its
# vector units round a square root and a division); on the two machines this was measured on, Adam: 3.57e-7 / 3.67e-7, Adadelta: 2.24e-7 /
# 2.50e-7; the bar is taken from the larger.  tests/test_refs64_feat_cpu.py asserts that the bar is between 4 and 6 times what it measures.
BAR_UPDATE = {'adam': 2e-6, 'adadelta': 1e-6}
# The update cases fix n = 2 * 4096 * 256 + 13, the start (p = 0, zero state) and BAR_SUM; the worst of 2 M chains of 6 - 10 roundings puts
# fp32 itself at 2.2e-7 .. 5.7e-7 of the max from float64 there (p of steps 2, 3: 2.9e-7 .. 3.2e-7; Adadelta's acc_delta: 5.5e-7 .. 5.7e-7), so the
# quarter that margin_ok asks everywhere else cannot hold; their precondition is that the fp32 CPU run stays within this share of the bar
UPDATE_MARGIN = 0.75

MISTAKES = ('last bin iteration dropped', 'last filter iteration dropped', 'clamp gradient kept', 'empty filter reads its neighbour',
            'one-pass variance in fp32', 'biased running variance', 'slope on the positive side', 'smooth l1 switches at 0.5',
            'bce without the -100 clamp', 'last chunk dropped', 'adam corrections in float')


def _t(v, dtype):
    return torch.as_tensor(v).detach().to(dtype)


# ---------------------------------------------------------------------------------------------
# filterbank
# ---------------------------------------------------------------------------------------------
def _runs_of_columns(M):
    """Per column of the 2-D array M: (offset, length) of the run from its first to its last non-zero row (0, 0 for a zero column)."""
    nzmask = M != 0
    any_ = nzmask.any(0)
    rows = np.arange(M.shape[0])[:, None]
    first = np.where(nzmask, rows, M.shape[0]).min(0)
    last = np.where(nzmask, rows, -1).max(0)
    off = np.where(any_, first, 0).astype(np.int64)
    ln = np.where(any_, last - first + 1, 0).astype(np.int64)
    return off, ln


def band_tables(W):
    """The banded forms re2e_fbank_fwd / _bwd take of an (F, NF) matrix, derived a second time: by filter ``off`` / ``len`` (NF,), ``taps``
    (NF, maxw) -- bins off[j] .. off[j] + len[j] - 1 of column j, zero beyond -- and by bin ``toff`` / ``tlen`` (F,), ``tw`` (F, maxc) --
    filters toff[b] .. of row b.  A run is first to last non-zero: an interior zero belongs to it; an all-zero column has offset 0 and
    length 0; maxw / maxc are the longest runs, at least 1."""
    Wn = np.asarray(W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else W, dtype=np.float32)
    out = {}
    for M, ko, kl, kw, km in ((Wn, 'off', 'len', 'taps', 'maxw'), (Wn.T, 'toff', 'tlen', 'tw', 'maxc')):
        off, ln = _runs_of_columns(M)
        width = max(int(ln.max()), 1)
        pos = off[:, None] + np.arange(width)[None, :]                                   # (columns, width) row index of each tap
        live = np.arange(width)[None, :] < ln[:, None]
        vals = np.where(live, M[np.minimum(pos, M.shape[0] - 1), np.arange(M.shape[1])[:, None]], 0.0).astype(np.float32)
        out.update({ko: off.astype(np.int32), kl: ln.astype(np.int32), kw: vals, km: width})
    return out


def _drop_last_iterations(W, by_bin):
    """W with what the LAST 8-wide iteration of each 32-wide tile contracts removed where that iteration is partial: forward (by_bin
    False) a tile of 32 filters walks the bins lo .. hi its filters cover from (lo // 8) * 8 in steps of 8; backward a tile of 32 bins
    walks the filters covering it the same way."""
    Wn = W.clone()
    M = Wn.t() if by_bin else Wn                      # (contracted axis, tiled axis) view
    off, ln = _runs_of_columns(M.numpy())
    for t0 in range(0, M.shape[1], 32):
        live = ln[t0:t0 + 32] > 0
        if not live.any():
            continue
        hi = int((off[t0:t0 + 32] + ln[t0:t0 + 32])[live].max())
        if hi % 8:
            M[hi - hi % 8:hi, t0:t0 + 32] = 0
    return Wn


def fbank_ref(x, W, cmvn=None, g_raw=None, g_norm=None, dtype=torch.float64, mistake=None):
    """x (rows, F), W (F, NF), cmvn (2, NF) or None, g_raw / g_norm (rows, NF) upstream gradients or None -> dict: pw = x^2 W (what
    pw_out holds: before the clamp), y_raw = log(p) with p[p <= 1e-7] = 1e-7 (a NaN is not clamped), y_norm = (y_raw + cmvn[0]) * cmvn[1],
    dx = d(sum y_raw g_raw + sum y_norm g_norm) / dx -- the in-place clamp passes no gradient."""
    xl = _t(x, dtype).clone().requires_grad_(True)
    Wd = _t(W, dtype)
    Wf = Wb = Wd
    if mistake == 'empty filter reads its neighbour':
        Wf = Wd.clone()
        for j in (Wd != 0).any(0).logical_not().nonzero().flatten().tolist():
            Wf[:, j] = Wd[:, j + 1 if j + 1 < Wd.shape[1] else j - 1]
        Wb = Wf
    elif mistake == 'last bin iteration dropped':
        Wf = _drop_last_iterations(Wd, False)
    elif mistake == 'last filter iteration dropped':
        Wb = _drop_last_iterations(Wd, True)
    pw = (xl * xl) @ Wf
    floor = torch.full_like(pw, CLAMP)
    fired = pw <= CLAMP
    p = torch.where(fired, floor, pw)
    if mistake == 'clamp gradient kept':
        p = p + (pw - pw.detach())                     # the value of the clamp, the gradient of the identity
    y = torch.log(p)
    out = dict(pw=pw.detach(), y_raw=y.detach())
    c = _t(cmvn, dtype) if cmvn is not None else None
    if c is not None:
        out['y_norm'] = ((y + c[0]) * c[1]).detach()
    if g_raw is None and g_norm is None:
        return out
    if Wb is Wf:
        L = 0.0
        if g_raw is not None:
            L = L + (y * _t(g_raw, dtype)).sum()
        if g_norm is not None:
            L = L + ((y + c[0]) * c[1] * _t(g_norm, dtype)).sum()
        L.backward()
        out['dx'] = xl.grad
    else:                                              # the backward's own table is the wrong one: its product written out
        gy = (_t(g_raw, dtype) if g_raw is not None else 0.0) + (_t(g_norm, dtype) * c[1] if g_norm is not None else 0.0)
        g = torch.where(fired, torch.zeros_like(pw), gy / pw).detach()
        out['dx'] = 2.0 * xl.detach() * (g @ Wb.t())
    return out


def logclamp_ref(z, cmvn=None, dy=None, dtype=torch.float64, mistake=None):
    """The element-wise tail of the trainable-matrix path: z (rows, N) = x^2 W from the GEMM engine -> y = log(z clamped as above)
    [-> (y + cmvn[0]) * cmvn[1]]; dz = dy [* cmvn[1]] / z, zero where the clamp fired."""
    zl = _t(z, dtype).clone().requires_grad_(True)
    p = torch.where(zl <= CLAMP, torch.full_like(zl, CLAMP), zl)
    if mistake == 'clamp gradient kept':
        p = p + (zl - zl.detach())
    y = torch.log(p)
    if cmvn is not None:
        c = _t(cmvn, dtype)
        y = (y + c[0]) * c[1]
    out = dict(y=y.detach())
    if dy is not None:
        (y * _t(dy, dtype)).sum().backward()
        out['dz'] = zl.grad
    return out


def cmvn_stats_ref(y, lens, dtype=torch.float64):
    """y (B, T, NF), lens (B,) -> per-column (sum, sum of squares) over the frames t < lens[b]."""
    yd = _t(y, dtype)
    valid = (torch.arange(yd.shape[1]).unsqueeze(0) < torch.as_tensor(lens).long().unsqueeze(1)).to(dtype).unsqueeze(2)
    return (yd * valid).sum((0, 1)), (yd * yd * valid).sum((0, 1))


def mel_fixture():
    """The (257, 80) mel matrix as tests/golden/fbank_tiny.npz holds it, with the fixture's input, CMVN and outputs."""
    return dict(np.load(os.path.join(GOLDEN, 'fbank_tiny.npz')))


def synth_bank(F, NF, seed):
    """A synthetic banded (F, NF) matrix with positive taps in [0.2, 1]: filter j starts near j (F - 32) / NF plus a jitter (offsets that are
    no multiple of 8), is 1 .. 32 bins long (spans over two and three 8-bin iterations), and
      - filter NF // 2 is 32 taps wide (MAXW) when F allows, filter 1 (when there is one) is all zero, filter NF // 3 has an interior zero,
      - at NF >= 24 twelve neighbouring filters share one offset: their bins are covered by more than 8 filters (two backward iterations),
      - the last 9 bins of F >= 40 and one bin inside are covered by no filter (at F = 520: a whole 32-bin tile and more, 480 .. 519)."""
    g = torch.Generator().manual_seed(seed)
    W = torch.zeros(F, NF)
    top = F - (40 if F == 520 else 9 if F >= 40 else 0)                 # first bin no filter may touch
    for j in range(NF):
        ln = int(torch.randint(1, min(32, top) + 1, (1,), generator=g))
        if j == NF // 2:
            ln = min(32, top)
        off = min(int(j * max(top - 32, 0) / NF) + int(torch.randint(0, 8, (1,), generator=g)), top - ln)
        W[off:off + ln, j] = 0.2 + 0.8 * torch.rand(ln, generator=g)
    if NF >= 24:
        o = int(W[:, NF // 4].nonzero()[0])
        for j in range(NF // 4, NF // 4 + 12):
            W[:, j] = 0
            W[o:o + 10, j] = 0.2 + 0.8 * torch.rand(10, generator=g)
    if NF > 3:
        j = NF // 3
        nz = W[:, j].nonzero().flatten()
        if len(nz) >= 3:
            W[int(nz[len(nz) // 2]), j] = 0
    if NF > 1:
        W[:, 1] = 0
    if F >= 40:
        W[F // 2] = 0
    return W


FBANK_BANKS = ('mel-257x80', 'synth-257x78', 'synth-256x33', 'synth-520x128', 'synth-40x5', 'synth-5x1')
FBANK_FRAMES = (1, 31, 32, 33, 70)
# (bank, frames, operand that sits 4 bytes off a 16-byte boundary or None): every bank at every frame count, then NF % 4 == 0 with one
# operand of the 16-byte path misaligned (the launcher must fall to the 4-byte loads)
FBANK_CASES = [(b, r, None) for b in FBANK_BANKS for r in FBANK_FRAMES] + \
              [('mel-257x80', 33, m) for m in ('pw', 'dy_raw', 'dy_norm', 'cmvn')] + [('synth-520x128', 70, 'pw'), ('synth-520x128', 33, 'cmvn')]
FBANK_FWD_OUTS = [tuple(bool(m >> k & 1) for k in range(3)) for m in range(1, 8)]        # (y_raw, y_norm, pw_out) present
FBANK_BWD_INS = [(True, False), (False, True), (True, True)]                               # (dy_raw, dy_norm) present


def fbank_case_id(row):
    return '%s-frames%d%s' % (row[0], row[1], '-%s-misaligned' % row[2] if row[2] else '')


def fbank_bank(name):
    if name.startswith('mel'):
        return torch.from_numpy(mel_fixture()['W']).float()
    F, NF = (int(v) for v in name.split('-')[1].split('x'))
    return synth_bank(F, NF, seed=7 * F + NF)


def bank_properties(W):
    """What a matrix makes the kernels do, as a set of names (tests/test_refs64_feat_cpu.py asserts that the table reaches them all)."""
    F, NF = W.shape
    b = band_tables(W)
    live = b['len'] > 0
    props = set()
    if (b['len'] == 32).any():
        props.add('a filter of MAXW taps')
    if (~live).any():
        props.add('an all-zero filter')
    if (b['tlen'] == 0).any():
        props.add('a bin no filter covers')
    if any((b['tlen'][t:t + 32] == 0).all() for t in range(0, F, 32)):
        props.add('a bin tile no filter covers')
    if (b['tlen'] > 8).any():
        props.add('a bin covered by more than 8 filters')
    if (b['off'][live] % 8 != 0).any():
        props.add('an offset off the 8-bin grid')
    if ((b['off'][live] + b['len'][live] - 1) // 8 - b['off'][live] // 8 >= 2).any():
        props.add('a filter over three 8-bin iterations')
    if ((b['taps'] == 0) & (np.arange(b['maxw'])[None, :] < b['len'][:, None])).any():
        props.add('an interior zero tap')
    for what, n in (('NF', NF), ('F', F)):
        if n % 32:
            props.add('%s %% 32 != 0' % what)
        if n > 32:
            props.add('%s in more than one tile' % what)
    props.add('NF %% 4 == %d' % (NF % 4))
    if NF == 128 and F == 520:
        props.add('both ABI maxima')
    return props


def fbank_case(row):
    """Inputs of a row, a function of (bank, frames): signed x with |x| in [10, 70] (every band power far above the clamp) except frame 0
    of frames >= 31 and frame 2 of frames >= 33, which are all zero (the clamp fires: log(1e-7), gradient 0), and frame 1 of frames
    >= 31, which is 1e-7 of that (the clamp fires on a non-zero x: a gradient that ignored it would be astronomically large).  Asserts the
    condition of the bars: no float64 band power in (1e-8, 1e-6)."""
    name, rows = row[0], row[1]
    W = fbank_bank(name)
    F, NF = W.shape
    g = torch.Generator().manual_seed(1000 * rows + F + NF)
    x = (10.0 + 20.0 * rnd(g, rows, F).abs()) * torch.where(torch.rand(rows, F, generator=g) < 0.5, -1.0, 1.0)
    if rows >= 31:
        x[0] = 0
        x[1] *= 1e-7
    if rows >= 33:
        x[2] = 0
    cmvn = torch.stack([10.0 + 4.0 * torch.rand(NF, generator=g), 0.3 + 0.3 * torch.rand(NF, generator=g)])
    case = dict(W=W, x=x, cmvn=cmvn, g_raw=rnd(g, rows, NF), g_norm=rnd(g, rows, NF), rows=rows, F=F, NF=NF)
    pw = (x.double() ** 2) @ W.double()
    assert not ((pw > 1e-8) & (pw < 1e-6)).any(), 'a band power sits where fp32 rounding decides whether the clamp fires'
    return case


def fbank_case_ref(case, ins=(True, True), dtype=torch.float64, mistake=None):
    return fbank_ref(case['x'], case['W'], case['cmvn'], case['g_raw'] if ins[0] else None, case['g_norm'] if ins[1] else None, dtype, mistake)


# (rows, N, with cmvn): exact zeros and values below the clamp in every case; the last is more than one sweep of the 8192 x 256 grid
LOGCLAMP_CASES = [(7, 80, True), (33, 65, False), (8192 + 3, 256, True), (8192 + 3, 256, False)]


def logclamp_case(rows, N):
    g = torch.Generator().manual_seed(rows + N)
    z = 0.05 + 30.0 * torch.rand(rows, N, generator=g) ** 2
    z[::5, ::3] = 0.0
    z[1::7, 1::4] = 1e-9
    assert not ((z > 1e-8) & (z < 1e-6)).any()
    cmvn = torch.stack([10.0 + 4.0 * torch.rand(N, generator=g), 0.3 + 0.3 * torch.rand(N, generator=g)])
    return dict(z=z, cmvn=cmvn, dy=rnd(g, rows, N))


# (B, T, NF, lens): two column blocks of 64 (one ragged at 65), lens with 0 and T
CMVN_CASES = [(4, 23, 80, (23, 0, 9, 1)), (3, 17, 65, (0, 17, 16))]


def cmvn_case(B, T, NF):
    g = torch.Generator().manual_seed(31 * T + NF)
    return 3.0 + 2.0 * rnd(g, B, T, NF)                 # log-filterbank-like: the sums do not cancel


# ---------------------------------------------------------------------------------------------
# BatchNorm + LeakyReLU over rows (P, C)
# ---------------------------------------------------------------------------------------------
def bn_chunks(P):
    """Row chunks of the partial kernels (csrc/elementwise.hip bn_chunks), rows per chunk."""
    c = min(512, max(1, (P + 255) // 256))
    return c, (P + c - 1) // c


def bn_lrelu_ref(x, gamma, beta, rm, rv, momentum=0.1, eps=1e-5, train=True, slope=0.2, dy=None, dgamma0=None, dbeta0=None, gbeta=0.0,
                 dtype=torch.float64, mistake=None):
    """x (P, C) -> dict: y = lrelu((x - mean) * invstd * gamma + beta), save_mean, save_invstd, running_mean, running_var (train: batch
    statistics, biased variance in invstd, the running variance takes the unbiased one, P / (P - 1); eval: the running statistics are
    the statistics and stay as they are); with ``dy``: dx (train: through the batch statistics), dgamma = gbeta * dgamma0 + sum dz xhat,
    dbeta = gbeta * dbeta0 + sum dz, dz = dy through the LeakyReLU."""
    xl = _t(x, dtype).clone().requires_grad_(True)
    ga, be = _t(gamma, dtype).clone().requires_grad_(True), _t(beta, dtype).clone().requires_grad_(True)
    rm_, rv_ = _t(rm, dtype), _t(rv, dtype)
    P = xl.shape[0]
    if train:
        xs = xl
        if mistake == 'last chunk dropped':
            chunks, rpc = bn_chunks(P)
            xs = xl[:(chunks - 1) * rpc] if chunks > 1 else xl
        mean = xs.sum(0) / P
        if mistake == 'one-pass variance in fp32':
            x32 = xs.detach().float()
            var = ((x32 * x32).sum(0) / P - (x32.sum(0) / P) ** 2).to(dtype) + 0.0 * mean
        else:
            var = ((xs - mean) ** 2).sum(0) / P
        unb = var.detach() * (P / (P - 1.0)) if P > 1 and mistake != 'biased running variance' else var.detach()
        new_rm, new_rv = (1.0 - momentum) * rm_ + momentum * mean.detach(), (1.0 - momentum) * rv_ + momentum * unb
    else:
        mean, var, new_rm, new_rv = rm_, rv_, rm_.clone(), rv_.clone()
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (xl - mean) * invstd
    v = xh * ga + be
    y = torch.where(v >= 0, slope * v, v) if mistake == 'slope on the positive side' else torch.where(v > 0, v, slope * v)
    out = dict(y=y.detach(), save_mean=mean.detach(), save_invstd=invstd.detach(), running_mean=new_rm, running_var=new_rv)
    if dy is not None:
        (y * _t(dy, dtype)).sum().backward()
        out['dx'] = xl.grad
        out['dgamma'] = ga.grad + (gbeta * _t(dgamma0, dtype) if gbeta != 0.0 else 0.0)
        out['dbeta'] = be.grad + (gbeta * _t(dbeta0, dtype) if gbeta != 0.0 else 0.0)
    return out


BN_C = (3, 4, 64, 68, 130)                      # scalar, float4, one full channel block, float4 / scalar over two blocks
BN_P = (2, 255, 257, 4353)                      # 1, 1, 2, 18 chunks
BN_P_LARGE = (16643, 131075)                    # 66 chunks; 512 chunks, beyond the cap (C = 4)
# (P, C, slope, gbeta, train, special): special in (None, 'x-misaligned', 'mean50')
BN_CASES = [(P, C, (0.2, 1.0)[(i + k) % 2], float((i + k) // 2 % 2), True, None) for i, P in enumerate(BN_P) for k, C in enumerate(BN_C)] + \
           [(16643, 4, 0.2, 1.0, True, None), (131075, 4, 0.2, 0.0, True, None), (131075, 4, 1.0, 1.0, True, None),
            (255, 64, 0.2, 0.0, True, 'x-misaligned'), (4353, 64, 0.2, 1.0, True, 'mean50'),
            (255, 3, 0.2, 0.0, False, None), (257, 64, 1.0, 0.0, False, None), (4353, 68, 0.2, 0.0, False, None)]
BN_QUANTITIES = (('y', BAR_BN_OUT), ('save_mean', BAR_BN_OUT), ('save_invstd', BAR_BN_OUT), ('running_mean', BAR_BN_OUT), ('running_var', BAR_BN_OUT),
                 ('dx', BAR_BN_GRAD), ('dgamma', BAR_BN_GRAD), ('dbeta', BAR_BN_GRAD))
BN_MOMENTUM, BN_EPS = 0.1, 1e-5
BN_FLIP_BAND = 1e-5                             # |y64| <= this of max |y64|: the LeakyReLU's derivative may legitimately flip in fp32
BN_SYNC_CASE = (257 * 8, 68, 0.2)               # rows split 3 : 5 between two ranks


def bn_case_id(row):
    P, C, slope, gbeta, train, special = row
    return 'P%d-C%d-slope%g-gbeta%g-%s%s' % (P, C, slope, gbeta, 'train' if train else 'eval', '-' + special if special else '')


def bn_case(P, C, special=None, slope=0.2):
    """x ~ 0.5 + 2 N(0,1) (test_bn_lrelu's), gamma ~ 1 + 0.3 N, beta ~ 0.3 N, running statistics away from (0, 1), dy ~ N(0,1).  P = 2: x ~ 0.003 N(0,1)
    -- with a spread far above sqrt(eps) the two normalised values are +-1 whatever x is and dx is the difference of two equal numbers,
    which no fp32 run resolves; around 0.5 the fp32 rounding of the mean alone is 2e-5 of such a spread.  'mean50': x ~ 50 + 0.5 N (a one-pass variance loses it).  With a slope
    other than 1, entries whose pre-activation lies within 1e-4 of the largest are moved away from zero, so that the share of entries
    where the derivative may flip (BN_FLIP_BAND) is zero."""
    g = torch.Generator().manual_seed(100003 * (P % 1009) + 17 * C + (5 if special == 'mean50' else 0))
    if special == 'mean50':
        x = 50.0 + 0.5 * rnd(g, P, C)
    elif P == 2:
        x = 0.003 * rnd(g, P, C)
    else:
        x = 0.5 + 2.0 * rnd(g, P, C)
    case = dict(gamma=1.0 + 0.3 * rnd(g, C), beta=0.3 * rnd(g, C), rm=0.2 * rnd(g, C), rv=0.5 + torch.rand(C, generator=g),
                dy=rnd(g, P, C), dgamma0=rnd(g, C), dbeta0=rnd(g, C))
    if slope != 1.0 and P > 2:
        for _ in range(20):
            v = bn_lrelu_ref(x, case['gamma'], case['beta'], case['rm'], case['rv'], slope=1.0)['y']
            close = v.abs() <= 1e-4 * v.abs().max()
            if not close.any():
                break
            x = torch.where(close, x + (0.01 if special == 'mean50' else 0.05) * torch.where(v >= 0, 1.0, -1.0).float(), x)
    case['x'] = x
    return case


def bn_flip_band(y64):
    """Entries the element-wise dx comparison leaves out."""
    return y64.abs() <= BN_FLIP_BAND * y64.abs().max()


def bn_case_ref(row, case, dtype=torch.float64, mistake=None):
    P, C, slope, gbeta, train, special = row
    return bn_lrelu_ref(case['x'], case['gamma'], case['beta'], case['rm'], case['rv'], BN_MOMENTUM, BN_EPS, train, slope,
                        case['dy'] if train else None, case['dgamma0'], case['dbeta0'], gbeta, dtype, mistake)


# ---------------------------------------------------------------------------------------------
# 2x2 / stride-2 ceil-mode max pool over NHWC, the VGG output pack: exact, no bar
# ---------------------------------------------------------------------------------------------
def pool_ref(x, relu_in=False):
    """x (NI, H, W, C) -> (values (NI, ceil(H/2), ceil(W/2), C), index bytes uint8).  The value is the maximum of the window's pixels
    inside the image, NaN when one of them is NaN (torch.max_pool2d); the byte is dy * 2 + dx of the first maximum in row-major order
    (of the last NaN, as torch's index), and with ``relu_in`` 4 wherever the maximum is not greater than 0 (a NaN included)."""
    NI, H, W, C = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xp = torch.full((NI, 2 * OH, 2 * OW, C), -INF, dtype=x.dtype)
    xp[:, :H, :W] = x
    inside = torch.zeros(2 * OH, 2 * OW, dtype=torch.bool)
    inside[:H, :W] = True
    best = xp[:, 0::2, 0::2].clone()
    bi = torch.zeros(best.shape, dtype=torch.uint8)
    for d in (1, 2, 3):
        v = xp[:, d >> 1::2, d & 1::2]
        take = ((v > best) | torch.isnan(v)) & inside[d >> 1::2, d & 1::2].reshape(1, OH, OW, 1)
        best = torch.where(take, v, best)
        bi = torch.where(take, torch.full_like(bi, d), bi)
    if relu_in:
        bi = torch.where(best > 0, bi, torch.full_like(bi, 4))
    return best, bi


def pool_bwd_ref(dout, idx, H, W):
    """din (NI, H, W, C): pixel (2 oy + dy, 2 ox + dx) takes dout[oy, ox] where the byte is dy * 2 + dx, else 0."""
    NI, OH, OW, C = dout.shape
    din = torch.zeros(NI, 2 * OH, 2 * OW, C, dtype=dout.dtype)
    for d in range(4):
        din[:, d >> 1::2, d & 1::2] = torch.where(idx == d, dout, torch.zeros_like(dout))
    return din[:, :H, :W].contiguous()


def pack_ref(src, lens, NI_total, n_off, base):
    """src (NI, T, Fq, C) -> rows n_off .. n_off + NI - 1 of a copy of ``base`` (T, NI_total, C * Fq): feature c * Fq + f, zero for
    t >= lens[n]; the other rows stay what they were."""
    NI, T, Fq, C = src.shape
    out = base.clone()
    live = (torch.arange(T).unsqueeze(0) < torch.as_tensor(lens).long().unsqueeze(1)).view(NI, T, 1, 1)
    out[:, n_off:n_off + NI] = torch.where(live, src, torch.zeros_like(src)).permute(1, 0, 3, 2).reshape(T, NI, C * Fq)
    return out


def pack_bwd_ref(dout, lens, NI, n_off, Fq, C):
    """dout (T, NI_total, C * Fq) -> din (NI, T, Fq, C), zero for t >= lens[n]."""
    T = dout.shape[0]
    d = dout[:, n_off:n_off + NI].reshape(T, NI, C, Fq).permute(1, 0, 3, 2)
    live = (torch.arange(T).unsqueeze(0) < torch.as_tensor(lens).long().unsqueeze(1)).view(NI, T, 1, 1)
    return torch.where(live, d, torch.zeros_like(d)).contiguous()


# (NI, H, W, C, index buffer 1 byte off a 4-byte boundary): scalar (C = 6, or the odd index pointer) and float4 (C = 8) kernels, odd H and W
# (ceil-mode windows at both edges), one row, one column, one pixel
POOL_CASES = [(3, 37, 21, 6, False), (3, 37, 21, 8, False), (2, 9, 7, 8, True), (2, 1, 9, 8, False), (2, 9, 1, 6, False), (1, 1, 1, 8, False),
              (2, 6, 4, 8, False)]


def pool_case(NI, H, W, C):
    """Rounded to halves (ties in most windows); window (0, 0) of image 0 all negative, window (0, 1) all zero (when there is one)."""
    g = torch.Generator().manual_seed(H * 100 + W * 10 + C)
    x = torch.round(rnd(g, NI, H, W, C) * 2) / 2
    x[0, :2, :2] = -torch.round(torch.rand(x[0, :2, :2].shape, generator=g) * 4 + 1) / 2
    if W > 2:
        x[0, :2, 2:4] = 0.0
    return x


def pool_nan_case(NI, H, W, C):
    """pool_case with a NaN in the first, in a middle and in the last position of three windows, windows of -inf, and a window holding
    +inf: what torch.max_pool2d propagates."""
    x = pool_case(NI, H, W, C)
    n = NI - 1
    x[n, 2, 2, 0] = NAN                               # first pixel of window (1, 1)
    x[n, 2, 5, 1] = NAN                               # second pixel of window (1, 2)
    x[n, H - 1, W - 1, C - 1] = NAN                   # the corner window: one pixel at odd H, W
    x[n, 4:6, 0:2, :] = -INF                          # window (2, 0), every channel
    x[n, 4, 2, 2] = INF
    x[n, 5, 3, 2] = NAN                               # +inf and a NaN behind it in one window: NaN
    return x


# (NI, T, Fq, C, NI_total, n_off, lens): the tiled kernel with a second branch's rows beside it, lens with 0 and T; a single branch; a
# frame whose Fq * (C + 1) floats exceed 48 KB of LDS (element-wise kernel)
PACK_CASES = [(3, 5, 4, 6, 7, 2, (5, 0, 3)), (2, 3, 5, 8, 2, 0, (3, 1)), (1, 2, 25, 512, 3, 1, (2,)), (2, 2, 25, 512, 2, 0, (1, 2))]


# ---------------------------------------------------------------------------------------------
# loss reductions
# ---------------------------------------------------------------------------------------------
L2, L1, SMOOTH_L1, BCE = 0, 1, 2, 3                 # RE2E_LOSS_*
BCE_EPS = float(np.float32(1e-12))                  # ATen's `constexpr float EPSILON = 1e-12`, a float in its double kernels too
LOSS_NAMES = ('l2', 'l1', 'smoothl1', 'bce')


def loss_ref(a, b_or_target, kind, gscale=None, scale=1.0, da0=None, beta=0.0, dtype=torch.float64, mistake=None):
    """a (n,), b_or_target: a tensor (n,) or a float -> (mean over n of the element loss, gradient (gscale or 1) * scale / n * d elem / da
    + beta * da0).  BCE is on probabilities: -(t log a + (1 - t) log(1 - a)) with both logarithms clamped at -100, gradient
    (a - t) / max(a (1 - a), 1e-12f) (ATen's binary_cross_entropy forward / backward)."""
    ad = _t(a, dtype)
    t = _t(b_or_target, dtype) if isinstance(b_or_target, torch.Tensor) else torch.full_like(ad, float(b_or_target))
    d = ad - t
    if kind == L2:
        elem, grad = d * d, 2.0 * d
    elif kind == L1:
        elem, grad = d.abs(), torch.sign(d)
    elif kind == SMOOTH_L1:
        knee = 0.5 if mistake == 'smooth l1 switches at 0.5' else 1.0
        inner = d.abs() < knee
        elem, grad = torch.where(inner, 0.5 * d * d, d.abs() - 0.5), torch.where(inner, d, torch.sign(d))
    else:
        la, l1a = torch.log(ad), torch.log(1.0 - ad)
        if mistake != 'bce without the -100 clamp':
            la, l1a = la.clamp(min=-100.0), l1a.clamp(min=-100.0)
        elem = -(t * la + (1.0 - t) * l1a)
        grad = (ad - t) / (ad * (1.0 - ad)).clamp(min=BCE_EPS)
    n = ad.numel()
    gs = float(gscale) if gscale is not None else 1.0
    da = grad * (gs * scale / n)
    if beta != 0.0:
        da = da + beta * _t(da0, dtype)
    return elem.sum() / n, da


LOSS_N = (1, 255, 4096, 4097, 1024 * 4096 + 5)     # one element; below / at / one past a workgroup's 4096; beyond the cap of 1024 workgroups
# (kind, n, target: 'tensor' / 'scalar' / 'soft' / 'edges', gscale present, beta)
LOSS_CASES = [(k, n, ('tensor', 'scalar')[(i + k) % 2], (i + k) % 2 == 0, float((i + k) // 2 % 2)) for k in (L2, L1, SMOOTH_L1) for i, n in enumerate(LOSS_N)] + \
             [(BCE, n, ('tensor', 'scalar', 'soft')[i % 3], i % 2 == 1, float(i // 2 % 2)) for i, n in enumerate(LOSS_N)] + \
             [(BCE, 255, 'edges', True, 0.0), (L1, 4097, 'scalar', False, 1.0), (SMOOTH_L1, 4097, 'tensor', True, 0.0)]
LOSS_SCALE, LOSS_GSCALE = 1.7, 0.6


def loss_case_id(row):
    kind, n, tk, gs, beta = row
    return '%s-n%d-%s%s-beta%g' % (LOSS_NAMES[kind], n, tk, '-gscale' if gs else '', beta)


def loss_case(row):
    """a, target (tensor or float), da0.  L1 / SmoothL1: a and b on a grid of 1/4, so that d is exactly 0 in a fifth of the entries
    and |d| exactly 1 in others (the sign of an fp32 difference is exact: no exclusion); BCE: a in (0.02, 0.98) against hard labels,
    a scalar label or a soft target in (0, 1); 'edges': a in {0, 1} against t in {0, 1}, all four pairs (values 0 or 100, gradients 0 or
    -+1e12)."""
    kind, n, tk, gs, beta = row
    g = torch.Generator().manual_seed(97 * kind + n % 100003 + len(tk))
    da0 = rnd(g, n)
    if kind == BCE:
        if tk == 'edges':
            a = (torch.arange(n) % 2).float()
            return dict(a=a, t=((torch.arange(n) // 2) % 2).float(), da0=da0)
        a = 0.02 + 0.96 * torch.rand(n, generator=g)
        t = {'tensor': (torch.rand(n, generator=g) < 0.5).float(), 'soft': 0.05 + 0.9 * torch.rand(n, generator=g), 'scalar': 1.0}[tk]
        return dict(a=a, t=t, da0=da0)
    if kind == L2:
        a = rnd(g, n, scale=2.0)
        return dict(a=a, t=rnd(g, n, scale=2.0) if tk == 'tensor' else 1.0, da0=da0)
    a = torch.round(rnd(g, n, scale=1.5) * 4) / 4
    t = torch.round(rnd(g, n, scale=1.5) * 4) / 4 if tk == 'tensor' else 0.25
    if n >= 5 and tk == 'tensor':
        t[0], t[1], t[2] = a[0], a[1] - 1.0, a[2] + 1.0
    elif n >= 5:
        a[0], a[1], a[2] = 0.25, 1.25, -0.75
    return dict(a=a, t=t, da0=da0)


def loss_case_ref(row, case, dtype=torch.float64, mistake=None):
    kind, n, tk, gs, beta = row
    return loss_ref(case['a'], case['t'], kind, LOSS_GSCALE if gs else None, LOSS_SCALE, case['da0'], beta, dtype, mistake)


# ---------------------------------------------------------------------------------------------
# gradient norm, clipping, updates
# ---------------------------------------------------------------------------------------------
def sumsq_ref(x, dtype=torch.float64):
    xd = _t(x, dtype)
    return (xd * xd).sum()


def clip_ref(sumsq, max_norm, dtype=torch.float64):
    """re2e_clip_coef: [norm, min(max_norm / (norm + 1e-6), 1), finite | norm, 1, finite]; a NaN or inf sum has finite = 0 in both triples
    (what the norm and the coefficient then hold is not part of the contract)."""
    n = torch.sqrt(_t(sumsq, dtype).reshape(()))
    c = max_norm / (n + 1e-6)
    coef = c if bool(c < 1.0) else torch.ones_like(c)
    fin = torch.tensor(1.0 if math.isfinite(float(n)) else 0.0, dtype=dtype)
    return torch.stack([n, coef, fin, n, torch.ones_like(n), fin])


def _coef(stats):
    """Clip coefficient of a stats triple, None when the update is to be skipped (stats[2] == 0)."""
    if stats is None:
        return 1.0
    if float(stats[2]) == 0.0:
        return None
    return stats[1]


def adadelta_ref(p, g, sq, acc, rho, eps, lr, stats=None, dtype=torch.float64):
    """One step of torch.optim.Adadelta from the given state on the gradient stats[1] * g -> (p, sq, acc); unchanged when stats[2] == 0."""
    p_, g_, sq_, acc_ = (_t(v, dtype).clone() for v in (p, g, sq, acc))
    coef = _coef(stats)
    if coef is None:
        return p_, sq_, acc_
    gr = g_ * (_t(coef, dtype) if isinstance(coef, torch.Tensor) else coef)
    v = sq_ * rho + gr * gr * (1.0 - rho)
    delta = torch.sqrt(acc_ + eps) / torch.sqrt(v + eps) * gr
    return p_ - lr * delta, v, acc_ * rho + delta * delta * (1.0 - rho)


def adam_ref(p, g, m, v, lr, b1, b2, eps, step, stats=None, dtype=torch.float64, mistake=None):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) at step count ``step`` from the given state -> (p, m, v).  The bias
    corrections are Python floats, as torch.optim.Adam computes them, in either dtype."""
    p_, g_, m_, v_ = (_t(t, dtype).clone() for t in (p, g, m, v))
    coef = _coef(stats)
    if coef is None:
        return p_, m_, v_
    gr = g_ * (_t(coef, dtype) if isinstance(coef, torch.Tensor) else coef)
    mi = m_ * b1 + (1.0 - b1) * gr
    vi = v_ * b2 + (1.0 - b2) * gr * gr
    if mistake == 'adam corrections in float':
        f = lambda b: float(np.float32(1.0) - np.power(np.float32(b), np.float32(step), dtype=np.float32))
        bc1, bc2 = f(b1), f(b2)
    else:
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = torch.sqrt(vi) / math.sqrt(bc2) + eps
    return p_ - (lr / bc1) * mi / denom, mi, vi


UPDATE_N = 2 * 4096 * 256 + 13                    # more than one sweep of the 8192 x 256 grid, odd tail
SUMSQ_CASES = [(3, False), (4099, False), (4099, True), (UPDATE_N, False), (UPDATE_N, True)]        # (n, 4 bytes off a 16-byte boundary)
CLIP_CASES = [(49.0, 5.0), (4.0, 5.0), (INF, 5.0), (NAN, 5.0)]                                       # (sum of squares, max_norm)
# stats given to an update: a clip coefficient below 1, the gate-only triple, none
UPDATE_STATS = {'clipped': [7.0, 0.37, 1.0], 'gate': [7.0, 1.0, 1.0], 'none': None}
ADADELTA_HYPER = dict(rho=0.95, eps=1e-8, lr=1.0)
ADAM_BETAS = ((0.5, 0.999), (0.9, 0.999))
ADAM_HYPER = dict(lr=1e-3, eps=1e-8)
# (optimizer, betas or None, stats key, start: 'zero' = steps 1, 2, 3 from p = 0 and zero state / 'step1000' = one step from a given state)
UPDATE_CASES = [('adadelta', None, s, 'zero') for s in UPDATE_STATS] + \
               [('adam', b, s, 'zero') for b in ADAM_BETAS for s in UPDATE_STATS] + [('adam', b, 'clipped', 'step1000') for b in ADAM_BETAS]


def update_case_id(row):
    return '%s%s-%s-%s' % (row[0], '-betas%g,%g' % row[1] if row[1] else '', row[2], row[3])


def update_grads(n=UPDATE_N):
    """Three gradients ~ 0.3 N(0,1) with |g| >= 1e-3 (Adam's first update is lr * g / (|g| + eps): eps = 1e-8 stays a correction), and a
    state for the step-1000 case: p ~ N(0,1), m ~ 0.1 N, v ~ 0.09 (0.5 + U)."""
    g = torch.Generator().manual_seed(11)
    gs = []
    for _ in range(3):
        x = rnd(g, n, scale=0.3)
        gs.append(torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x))
    return gs, dict(p=rnd(g, n), m=rnd(g, n, scale=0.1), v=0.09 * (0.5 + torch.rand(n, generator=g)))


def update_run(row, grads, state, dtype=torch.float64, mistake=None):
    """The steps of a row through adam_ref / adadelta_ref -> list of (p, s1, s2) after each step."""
    opt, betas, sk, start = row
    st = torch.tensor(UPDATE_STATS[sk]) if UPDATE_STATS[sk] is not None else None
    n = grads[0].numel()
    if start == 'zero':
        cur, steps = (torch.zeros(n), torch.zeros(n), torch.zeros(n)), (1, 2, 3)
    else:
        cur, steps = (state['p'], state['m'], state['v']), (1000,)
    out = []
    for k, step in enumerate(steps):
        if opt == 'adam':
            cur = adam_ref(cur[0], grads[k], cur[1], cur[2], ADAM_HYPER['lr'], betas[0], betas[1], ADAM_HYPER['eps'], step, st, dtype, mistake)
        else:
            cur = adadelta_ref(cur[0], grads[k], cur[1], cur[2], ADADELTA_HYPER['rho'], ADADELTA_HYPER['eps'], ADADELTA_HYPER['lr'], st, dtype)
        out.append(cur)
    return out


def update_bar(row, k, q):
    """Bar of quantity q (0: p, 1 / 2: the state tensors) after the k-th step of a row."""
    return BAR_UPDATE[row[0]] if is_first_update(row, k, q) else BAR_SUM


def is_first_update(row, k, q):
    """p after step 1 from p = 0 and zero state."""
    return q == 0 and k == 0 and row[3] == 'zero'
