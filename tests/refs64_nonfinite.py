"""Float64 reference of what NaN and +-inf become in the activation epilogues and the loss reductions, and the poisoned inputs of
tests/test_nonfinite_kernels_gpu.py.

Plain torch on the CPU, nothing imported from the product or from ``oracle``.  The trainer's only defence against a poisoned step is its
grad-norm gate, which works only if a NaN that enters a layer is still a NaN when it leaves; so every kernel form of
refs64_gemm.DENSE_CASES and refs64_conv.CONV_CASES runs once more on its own case with a few elements of the activations operand replaced
(``poison_dense`` / ``poison_conv``), and the stand-alone pointwise kernels run on small tables.  torch defines the semantics: ``relu``,
``leaky_relu``, ``tanh``, ``sigmoid``, ``+``; the expected result is refs64_gemm.dense_ref / refs64_conv.case_ref on the poisoned case
(``dense_expected`` / ``conv_expected``), tests/test_refs64_nonfinite_cpu.py pins both to F.linear / F.conv2d and torch's activations.

Placement.  Dense: NaN, +inf, -inf and a NaN in the last logical row, each in a different output row, so that every output sees at most one
non-finite term and the expected pattern is exact; the first NaN sits in the middle K slice of the row's declared plan, +inf at k = 0, the
others at k = K - 1.  Mask-epilogue rows take them inside and beyond ``lens`` (a fifth element, a NaN beyond ``lens``, where the four leave
none there).  Convolutions: a NaN in the last pixel and last channel, a NaN in the middle; +inf and -inf only where a pixel exists whose
receptive field (forward, data gradient: k pixels either way; weight gradient: the output channel) meets no other poisoned element's --
the 5 x 3 maps of the table have room for the two NaNs alone, whose fields may meet (NaN + NaN is NaN in any order).  In a weight gradient
+-inf also keep to pixels none of whose taps is padding: 0 x inf is a NaN that a kernel which skips padding does not form.

``MISTAKES`` are applied inside the reference, as in the sibling modules.  'leaky relu by max(v, 0.2 v)' is listed because it is the
obvious sibling of 'relu by fmax', but it is NO mistake: max(v, 0.2 v) and fmax(v, 0.2 v) equal leaky_relu on every float, NaN and both
infinities included, so it applies to no case and tests/test_refs64_nonfinite_cpu.py asserts the equality instead.

Differences recorded and not asserted:
  * a non-finite SAVED OUTPUT in the backward kernels (re2e_act_bwd with y = NaN): torch's threshold_backward passes the gradient where
    the kernels write 0.  The forward has already carried that NaN to the loss, so the gate fires either way.
  * F.binary_cross_entropy itself REFUSES a NaN probability on the CPU ('all elements of input should be between 0 and 1'); ``bce_ref``
    is ATen's formula written out, pinned to F.binary_cross_entropy wherever that runs, and NaN at a NaN probability, which is what
    the formula gives and what the gate needs.
  * the running maxima of the softmax / log-sum-exp kernels (ctc.hip, seqloss.hip, attloc.hip, attstep.hip, rnnlm.hip, wordlm.hip) use
    fmaxf and drop a NaN from the MAXIMUM; the NaN still reaches the sum through exp(x - m).  Not covered here.
"""
import contextlib

import torch
import torch.nn.functional as F

import refs64_conv as C
import refs64_gemm as G
from refs64_feat import BAR_FBANK_OUT, BAR_LOSS          # noqa: F401  (the bars of the pointwise tables: 1e-5 of the max)

NAN, INF = float('nan'), float('inf')
ACT_NONE, ACT_TANH, ACT_RELU, ACT_LRELU, ACT_SIGMOID, ACT_MASK = range(6)          # include/re2e.h RE2E_ACT_*
ACTS = (ACT_TANH, ACT_RELU, ACT_LRELU, ACT_SIGMOID)
L2, L1, SMOOTH_L1, BCE = 0, 1, 2, 3          # RE2E_LOSS_*

MISTAKES = {
    'relu by fmax': 'ReLU as fmax(v, 0): NaN -> 0',
    'relu as max(v, 0 v)': 'ReLU as fmax(v, 0 * v): -inf stays -inf (0 * -inf is NaN, which fmax drops)',
    'leaky relu by max(v, 0.2 v)': 'LeakyReLU as fmax(v, 0.2 v): equal to leaky_relu on every float (see the module docstring); applies nowhere',
    'log clamp by fmax': 'the BCE logarithms clamped by fmax(log a, -100): a NaN probability costs 100',
    'poisoned slice dropped from a split sum': 'the K slice (dense) or the image row (weight gradient) that holds the first NaN left out of the sum',
    'tail row not written': 'the last output row / pixel / output channel keeps its prior content',
}


def act_ref(v, act, mistake=None):
    """torch's activation of RE2E_ACT_* ``act`` (relu, leaky_relu(0.2), tanh, sigmoid), or a mistaken variant."""
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_RELU:
        if mistake == 'relu by fmax':
            return torch.fmax(v, torch.zeros_like(v))
        if mistake == 'relu as max(v, 0 v)':
            return torch.fmax(v, 0 * v)
        return torch.relu(v)
    if act == ACT_LRELU:
        if mistake == 'leaky relu by max(v, 0.2 v)':
            return torch.fmax(v, 0.2 * v)
        return F.leaky_relu(v, 0.2)
    if act in (ACT_SIGMOID, ACT_MASK):
        return torch.sigmoid(v)
    assert act == ACT_NONE
    return v


@contextlib.contextmanager
def _acts(mistake):
    """The activation of both sibling references replaced by ``act_ref`` (their own, clamp(min=0) and where(v > 0, v, 0.2 v), treat NaN and
    +-inf as torch's modules do -- tests/test_refs64_nonfinite_cpu.py -- but the mistakes need a place to go)."""
    saved = G._act, C._act
    G._act = C._act = lambda v, act: act_ref(v, act, mistake)
    try:
        yield
    finally:
        G._act, C._act = saved


def same_pattern(a, b):
    """NaNs in the same places, infinities in the same places with the same signs."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return bool(torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isposinf(a), torch.isposinf(b)) and torch.equal(torch.isneginf(a), torch.isneginf(b)))


def finite_err(got, ref, scale=None):
    """max |got - ref| over the elements that are finite in BOTH, over ``scale`` (default: the largest finite |ref|)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    fin = torch.isfinite(ref) & torch.isfinite(got)
    if not fin.any():
        return 0.0
    scale = ref[fin].abs().max().item() if scale is None else scale
    e = (got[fin] - ref[fin]).abs().max().item()
    return e / scale if scale > 0 else (0.0 if e == 0 else INF)


# ---------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------
def _dense_rows(row):
    """[(kind, value, logical output row)]"""
    M = row.M
    if row.act != ACT_MASK:
        rows = [M // 3, M // 2, 2 * M // 3, M - 1]
        assert M >= 5 and len(set(rows)) == 4, row
        return list(zip(('nan', '+inf', '-inf', 'nan_last'), (NAN, INF, -INF, NAN), rows))
    live = [r for r in range(M - 1) if r % row.T < row.lens[r // row.T]]
    dead = [r for r in range(M - 1) if r % row.T >= row.lens[r // row.T]]
    assert len(live) >= 3 and len(dead) >= 2, ('a mask row needs frames inside and beyond lens', row)
    spots = [('nan', NAN, live[len(live) // 2]), ('+inf', INF, dead[len(dead) // 2]), ('-inf', -INF, live[len(live) // 3]), ('nan_last', NAN, M - 1)]
    if (M - 1) % row.T < row.lens[(M - 1) // row.T]:          # the last frame is inside lens: one more NaN beyond them
        spots.append(('nan_beyond', NAN, dead[0] if dead[0] != spots[1][2] else dead[1]))
    assert len({s[2] for s in spots}) == len(spots)
    return spots


def poison_dense(row, case):
    """A copy of refs64_gemm.dense_case(row) with the elements of A above replaced -> the case, with 'poison': [(kind, output row, k)].
    Weights, biases and the prior content of C stay as they are."""
    sl = G.k_slices(row, row.plan)
    k0, k1 = sl[len(sl) // 2]
    ks = {'nan': (k0 + k1) // 2, '+inf': 0, '-inf': row.K - 1, 'nan_last': row.K - 1, 'nan_beyond': row.K // 2}
    A = case['A'].clone()
    m = case['map']
    poison = []
    for kind, value, r in _dense_rows(row):
        k = ks[kind]
        if row.op == 'tn':
            pk = int(m[k]) if row.entry == 'tn_rows' else k
            assert row.entry != 'tn_rows' or pk in set(m.tolist()), 'the poisoned row of the contraction is one the map keeps'
            A[pk, r] = value
        else:
            pr = int(m[r]) if row.entry == 'nt_rows' else r
            assert row.entry != 'nt_rows' or pr in set(m.tolist()), 'the poisoned output row is one the map keeps'
            A[pr, k] = value
        poison.append((kind, r, k))
    assert int((~torch.isfinite(A)).sum()) == len(poison) and torch.isfinite(case['B']).all()
    for kind, _, k in poison:          # what multiplies an infinity is not zero (the largest matrices of the table hold a few exact zeros elsewhere)
        Bk = case['B'][:, k] if row.op == 'nt' else case['B'][int(m[k]) if row.entry == 'tn_rows' else k]
        assert (Bk != 0).all(), (kind, k)
    out = dict(case)
    out.update(A=A, poison=poison)
    return out


def dense_rows(row, case):
    """The logical output rows the poisoned reference is evaluated on: all of them, or (rows too large for that, refs64_gemm.yard_rows) the
    poisoned rows and the yardstick sample; the last row comes last."""
    sample = G.yard_rows(row)
    if sample is None:
        return list(range(row.M))
    return sorted(set(sample) | {r for _, r, _ in case['poison']})


def dense_expected(row, case, clean, dtype=torch.float64, mistake=None, rows=None):
    """refs64_gemm.dense_ref on the poisoned case over ``rows`` (default dense_rows) -> dict(C, [mask_out], scale, rows); scale is the clean
    case's largest |op(A) op(B)| over the same rows, the unit of the row's bar."""
    rows = dense_rows(row, case) if rows is None else rows
    assert rows[-1] == row.M - 1
    c = case
    if mistake == 'poisoned slice dropped from a split sum':
        sl = G.k_slices(row, row.plan)
        k0, k1 = sl[len(sl) // 2]
        assert len(sl) > 1 and k0 <= [p for p in case['poison'] if p[0] == 'nan'][0][2] < k1
        A = case['A'].clone()
        ks = torch.arange(k0, k1)
        if row.op == 'tn':
            A[case['map'][ks] if row.entry == 'tn_rows' else ks] = 0
        else:
            A[:, ks] = 0
        c = dict(case, A=A)
    with _acts(mistake):
        out = G.dense_ref(row, c, dtype, rows=rows, plan=row.plan)
    if mistake == 'tail row not written':
        m = case['map']
        prior = case['C0'][int(m[row.M - 1]) if row.entry == 'nt_rows' else row.M - 1]
        out['C'][-1] = prior.to(dtype)
        if 'mask_out' in out:
            out['mask_out'][-1] = case['mask0'][row.M - 1].to(dtype)
    out['scale'] = G.dense_ref(row, clean, rows=rows, plan=row.plan)['scale']
    out['rows'] = rows
    return out


def dense_mistakes_of(row):
    m = []
    if row.act != ACT_MASK or (row.M - 1) % row.T < row.lens[(row.M - 1) // row.T]:          # (a last frame beyond lens holds a zero either way)
        m.append('tail row not written')
    if row.act == ACT_RELU:
        m += ['relu by fmax', 'relu as max(v, 0 v)']
    if len(G.k_slices(row, row.plan)) > 1:
        m.append('poisoned slice dropped from a split sum')
    return m


# ---------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------
def operand_of(row):
    return 'x' if row.direction == C.FWD else 'dz'


def _interior(row, oh, ow):
    """No tap of output pixel (oh, ow) is padding."""
    ok = lambda o, size: o * row.stride - row.pad >= 0 and o * row.stride - row.pad + row.k - 1 < size
    return ok(oh, row.H) and ok(ow, row.W)


def poison_conv(row, case):
    """A copy of refs64_conv.conv_case(row) with elements of the activations operand (x forward, dz in both gradient directions) replaced
    -> the case, with 'poison': [(kind, (n, h, w, c))].  Weights and bias stay as they are."""
    name = operand_of(row)
    t = case[name].clone()
    N, GH, GW, CH = t.shape
    spots = [('nan_last', NAN, (N - 1, GH - 1, GW - 1, CH - 1)), ('nan', NAN, (0, GH // 2, GW // 2, 0))]
    if row.direction == C.WGRAD:
        free = [c for c in range(1, CH - 1)]          # an output channel of its own
        pix = [(n, h, w) for n in range(N) for h in range(GH) for w in range(GW) if _interior(row, h, w)]
        for kind, value in (('+inf', INF), ('-inf', -INF)):
            if free and pix:
                spots.append((kind, value, pix[len(pix) // 3 if value > 0 else 2 * len(pix) // 3] + (free.pop(0),)))
    else:
        def clear(p):
            return all(p[0] != q[0] or abs(p[1] - q[1]) >= row.k or abs(p[2] - q[2]) >= row.k for _, _, q in spots)
        for kind, value in (('+inf', INF), ('-inf', -INF)):
            for n in range(N):
                hit = next(((n, h, w) for h in range(GH) for w in range(GW) if clear((n, h, w))), None)
                if hit is not None:
                    spots.append((kind, value, hit + (CH // 2,)))
                    break
    for _, value, idx in spots:
        t[idx] = value
    assert int((~torch.isfinite(t)).sum()) == len(spots) or spots[0][2] == spots[1][2]
    assert torch.isfinite(case['w']).all() and (case['w'] != 0).all()
    out = dict(case)
    out[name] = t
    out['poison'] = [(kind, idx) for kind, _, idx in spots]
    return out


def conv_expected(row, case, dtype=torch.float64, mistake=None):
    """refs64_conv.case_ref on the poisoned case -> tensor (pooled rows: (values, index bytes))."""
    c = case
    if mistake == 'poisoned slice dropped from a split sum':
        assert row.direction == C.WGRAD
        n, h, _, _ = [p for p in case['poison'] if p[0] == 'nan'][0][1]
        dz = case['dz'].clone()
        dz[n, h] = 0
        c = dict(case, dz=dz)
    with _acts(mistake):
        out = C.case_ref(row, c, dtype)
    if mistake == 'tail row not written':
        o = out[0] if row.flags & C.F_POOL else out
        if row.direction == C.WGRAD:
            o[-1] = case['dW0'][-1].to(dtype) if row.beta else 0
        else:
            o[-1, -1, -1] = case['y0'][-1, -1, -1].to(dtype) if row.beta and row.direction == C.FWD else 0
    return out


def conv_mistakes_of(row, case):
    m = ['tail row not written']
    kinds = {p[0] for p in case['poison']}
    if row.direction == C.FWD and row.act == ACT_RELU:
        m.append('relu by fmax')
        if '-inf' in kinds and not row.flags & C.F_POOL:          # (a pool window hides a -inf behind the zeros beside it)
            m.append('relu as max(v, 0 v)')
    if row.direction == C.WGRAD and row.Cout > 1:          # (one output channel: the NaN of the last pixel is in every sum)
        m.append('poisoned slice dropped from a split sum')
    return m


def touched(row, case):
    """Bool tensor over the row's output: where a Winograd kernel MAY hold a non-finite value -- the 2x2 output tiles (forward, data
    gradient; the pooled pixels they feed) whose input patch holds a poisoned element, the output channels (weight gradient) one sits in."""
    bare = row._replace(act=ACT_NONE, flags=row.flags & ~(C.F_POOL | C.F_MASK | C.F_BIAS), beta=0)
    hit = ~torch.isfinite(C.case_ref(bare, case))
    if row.direction == C.WGRAD:
        return hit.flatten(1).any(1)[:, None, None, None].expand_as(hit).clone()
    N, OH, OW, K = hit.shape
    ty, tx = (OH + 1) // 2, (OW + 1) // 2
    tiles = F.pad(hit, (0, 0, 0, 2 * tx - OW, 0, 2 * ty - OH)).view(N, ty, 2, tx, 2, K).any(4).any(2)
    if row.flags & C.F_POOL:
        return tiles
    return tiles[:, :, None, :, None, :].expand(N, ty, 2, tx, 2, K).reshape(N, 2 * ty, 2 * tx, K)[:, :OH, :OW].clone()


# ---------------------------------------------------------------------------------------------
# the remaining activations at every epilogue site: the smallest table row of the site, its shape, every other activation its entry point takes
# ---------------------------------------------------------------------------------------------
def dense_site_of(row):
    f = row.form
    if row.act == ACT_MASK or f[0] == 'below_plan':
        return None          # (the mask epilogue has one activation; re2e_gemm_skinny2 and the fallback take what their table rows run)
    if f[0] == 'skinny_wg':
        return 'skinny'
    if f[0] == 'pipeline':
        return 'pipeline ' + f[2]
    return 'engine ' + ('beta = 1' if row.beta and f[4] == 'one' else 'one slice' if f[4] == 'one' else 'split' if f[4] == 'split' else 'zx')


def dense_sites():
    """{site: the smallest DENSE_CASES row of it}"""
    best = {}
    for row in G.DENSE_CASES:
        s = dense_site_of(row)
        if s is not None and (s not in best or row.M * row.N * row.K < best[s].M * best[s].N * best[s].K):
            best[s] = row
    return best


def dense_variants():
    """[(site, the row with another activation)].  The plan looks at the activation in two places only, and both are left out here: the skinny
    route serves products WITHOUT one (with one, M <= 32 goes to the engine's 32x128 tile), and that tile only products WITH one."""
    out = []
    for site, row in sorted(dense_sites().items()):
        if site == 'skinny':
            continue
        for act in (ACT_NONE,) + ACTS:
            if act != row.act and not (act == ACT_NONE and row.plan.get('tile') == '32x128x32'):
                out.append((site, row._replace(act=act)))
    return out


def conv_site_of(row):
    if row.direction != C.FWD or row.flags & C.F_POOL:
        return None
    f = row.form
    if f[0] in ('cin1_fwd', 'cout1_rows', 'halo'):
        return f[0]
    if f[0] == 'cout1':
        return 'cout1 generic' if f[3:] == (0, 0, 0) else 'cout1 fixed taps'
    if f[0] in ('engine', 'pipeline', 'wino3x3'):
        return f[0]
    return None          # (F(2x2,4x4) has no epilogue beyond its output transform)


def conv_variants():
    """[(site, the row with another activation)]: re2e_conv_igemm takes none / ReLU / LeakyReLU (the halo kernel none / ReLU: a LeakyReLU
    layer of its shapes is planned onto the engine), re2e_conv3x3_wino none / ReLU."""
    best = {}
    for row in C.CONV_CASES:
        s = conv_site_of(row)
        size = lambda r: r.N * r.H * r.W * r.Cin * r.Cout
        if s is not None and (s not in best or size(row) < size(best[s])):
            best[s] = row
    out = []
    for site, row in sorted(best.items()):
        for act in (ACT_NONE, ACT_RELU) if site in ('wino3x3', 'halo') else (ACT_NONE, ACT_RELU, ACT_LRELU):
            if act != row.act:
                out.append((site, row._replace(act=act)))
    return out


def same_site(base_form, form):
    """The form a variant's plan names is the site's: the halo kernel's form carries its ReLU flag, which an activation changes by design."""
    if base_form[0] == 'halo':
        return form[:4] == base_form[:4] and form[5:] == base_form[5:]
    return form == base_form


# ---------------------------------------------------------------------------------------------
# pointwise tables
# ---------------------------------------------------------------------------------------------
SPECIALS = (NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, 0.25, -0.25, 20.0, -20.0, 100.0, -100.0)


def act_table(n):
    """n inputs of re2e_act_fwd: the specials, then N(0, 2) values, the pattern repeated (a NaN is also the last element)."""
    g = torch.Generator().manual_seed(n)
    base = torch.cat([torch.tensor(SPECIALS), rnd2(g, 4099 - len(SPECIALS))])
    x = base.repeat(-(-n // base.numel()))[:n].clone()
    x[-1] = NAN
    return x


def rnd2(g, *shape):
    return torch.randn(*shape, generator=g) * 2.0


def act_bwd_table(M, N):
    """(dy, y) of re2e_act_bwd / re2e_act_bwd_colsum, M x N: y finite in (-0.95, 0.95) with exact zeros and both signs (a saved output of
    any of the four activations' backward formulas); dy non-finite in four columns -- a NaN, +inf alone, -inf alone, +inf and -inf -- and in
    the last element; the other columns finite."""
    g = torch.Generator().manual_seed(M * 131 + N)
    y = (torch.rand(M, N, generator=g) * 1.9 - 0.95)
    y[::5, ::3] = 0.0
    dy = torch.randn(M, N, generator=g)
    assert N >= 6 and M >= 4
    dy[M // 2, 0] = NAN
    dy[1, 1] = INF
    dy[M - 2, 2] = -INF
    dy[0, 3], dy[M - 1, 3] = INF, -INF
    dy[M - 1, N - 1] = NAN
    y[M // 2, 0], y[1, 1], y[M - 2, 2], y[0, 3], y[M - 1, 3], y[M - 1, N - 1] = 0.5, 0.25, 0.75, 0.5, 0.5, 0.3          # the gradient passes there
    return dy, y


def act_bwd_ref(dy, y, act, dtype=torch.float64):
    """dz = dy act'(.) from the saved OUTPUT y, as torch's tanh_backward / sigmoid_backward / threshold_backward / leaky_relu_backward write
    it (finite y; see the module docstring for a non-finite one) -> (dz, its column sums)."""
    dy, y = dy.to(dtype), y.to(dtype)
    if act == ACT_TANH:
        dz = dy * (1 - y * y)
    elif act == ACT_SIGMOID:
        dz = dy * (1 - y) * y
    elif act == ACT_RELU:
        dz = torch.where(y > 0, dy, torch.zeros_like(dy))
    else:
        assert act == ACT_LRELU
        dz = torch.where(y > 0, dy, 0.2 * dy)
    return dz, dz.sum(0)


def fill_table(N):
    g = torch.Generator().manual_seed(N)
    v = torch.randn(N, generator=g)
    v[1], v[N // 2], v[N - 2], v[N - 1] = NAN, INF, -INF, NAN
    return v


LOSS_N = 301


def loss_table(kind, poison):
    """(a, t) of re2e_loss_fwd / re2e_loss_bwd, LOSS_N elements.  poison: 'finite', 'nan' (NaN, +inf and -inf differences / a NaN
    probability) or 'inf' (infinite differences, no NaN; L1, L2, smooth-L1 only).  BCE: every a of {0, 1, 1e-45, 1 - 2^-24} (and NaN)
    against every t of {0, 1, 0.3}, the rest probabilities in (0.02, 0.98)."""
    g = torch.Generator().manual_seed(kind * 7 + len(poison))
    if kind == BCE:
        assert poison in ('finite', 'nan')
        a = torch.rand(LOSS_N, generator=g) * 0.96 + 0.02
        t = torch.rand(LOSS_N, generator=g)
        i = 3
        for av in (0.0, 1.0, 1e-45, 1.0 - 2.0 ** -24) + ((NAN,) if poison == 'nan' else ()):
            for tv in (0.0, 1.0, 0.3):
                a[i], t[i] = av, tv
                i += 17
        if poison == 'nan':
            a[-1] = NAN
        return a, t
    a, t = torch.randn(LOSS_N, generator=g) * 1.5, torch.randn(LOSS_N, generator=g)
    a[::7] = t[::7]          # d = 0 exactly
    a[5], a[6] = t[5] + 1.0, t[6] - 1.0          # |d| = 1: the smooth-L1 branch point
    if poison != 'finite':
        a[11], a[150] = INF, -INF
    if poison == 'nan':
        a[20], a[-1] = NAN, NAN
    return a, t


def bce_ref(a, t, dtype=torch.float64, mistake=None):
    """ATen's binary_cross_entropy written out, per element -> (loss terms, d (mean loss) / d a): -(t max(log a, -100) + (1 - t) max(log(1 - a),
    -100)) with a NaN kept (see the module docstring), and (a - t) / max(a (1 - a), 1e-12) / n."""
    a, t = a.to(dtype), t.to(dtype)
    if mistake == 'log clamp by fmax':
        clamp = lambda v: torch.fmax(v, torch.full_like(v, -100.0))
    else:
        clamp = lambda v: torch.where(v < -100.0, torch.full_like(v, -100.0), v)
    val = -(t * clamp(torch.log(a)) + (1 - t) * clamp(torch.log1p(-a)))
    den = a * (1 - a)
    eps = torch.tensor(1e-12, dtype=torch.float32).item()          # ATen's EPSILON is a float constant
    grad = (a - t) / torch.where(den < eps, torch.full_like(den, eps), den) / a.numel()
    return val, grad


def loss_ref(kind, a, t, dtype=torch.float64, mistake=None):
    """-> (the mean loss, its gradient with respect to a): F.mse_loss / F.l1_loss / F.smooth_l1_loss and autograd; BCE: bce_ref."""
    if kind == BCE:
        val, grad = bce_ref(a, t, dtype, mistake)
        return val.mean(), grad
    fn = {L2: F.mse_loss, L1: F.l1_loss, SMOOTH_L1: F.smooth_l1_loss}[kind]
    x = a.to(dtype).clone().requires_grad_(True)
    loss = fn(x, t.to(dtype))
    loss.backward()
    return loss.detach(), x.grad
