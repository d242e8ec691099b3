"""tests/refs64_ops.py on the CPU: every new restatement pinned to torch's own module in double, the precondition of every bar
(``margin_ok``) on every row, the closure of ``OPS`` over the autograd Functions of robust_e2e_gan_amd/ops.py, and the sensitivity of
``check_protocol`` to six fabricated mistakes."""
import functools
import inspect

import pytest
import torch

import refs64 as R
import refs64_ops as O

D = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert R.rel_err(a, b) <= tol, R.rel_err(a, b)


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# restatements against torch.nn in double
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [None, 'tanh', 'relu', 'sigmoid', 'lrelu'])
def test_linear_ref_is_nn_linear(act):
    g = _g(1)
    m = torch.nn.Linear(12, 8).to(D)
    x = R.rnd(g, 3, 5, 12).to(D)
    f = {None: lambda v: v, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid, 'lrelu': torch.nn.LeakyReLU(0.2)}[act]
    _close(O.linear_ref(x, m.weight, m.bias, act), f(m(x)))
    # ragged time-major rows: the valid rows are the module's, the padded ones what the module gives for a zero frame
    valid = O.RR.valid_mask([3, 2, 1, 3, 1], 3)                      # x as (T, B, K) = (3, 5, 12)
    x0 = x * valid.unsqueeze(-1).to(D)
    _close(O.linear_ref(x, m.weight, m.bias, act, valid), f(m(x0)))


def test_linear_2bias_ref_is_nn_linear_plus_a_bias():
    g = _g(2)
    m = torch.nn.Linear(10, 8).to(D)
    x, b2 = R.rnd(g, 4, 3, 10).to(D), R.rnd(g, 8).to(D)
    _close(O.linear_2bias_ref(x, m.weight, m.bias, b2), m(x) + b2)


def test_fbank_dense_and_mask_refs_written_out():
    g = _g(3)
    x, W = R.rnd(g, 2, 5, 9).to(D), torch.rand(9, 4, generator=g).to(D)
    cm = torch.stack([torch.linspace(1, 2, 4), torch.linspace(0.3, 0.6, 4)]).to(D)
    z = torch.einsum('btf,fn->btn', x ** 2, W)
    z[0, 0, 0] = 0.0                                             # a clamped element
    x[0, 0] = 0.0
    want = torch.log(torch.where(torch.einsum('btf,fn->btn', x ** 2, W) <= 1e-7, torch.full_like(z, 1e-7), torch.einsum('btf,fn->btn', x ** 2, W)))
    _close(O.fbank_dense_ref(x, W), want)
    _close(O.fbank_dense_ref(x, W, cm), (want + cm[0]) * cm[1])
    m = torch.nn.Linear(16, 7, bias=False).to(D)
    proj, mix, lens = R.rnd(g, 3, 11, 16).to(D), R.rnd(g, 3, 11, 7).abs().to(D), [11, 7, 4]
    want = torch.sigmoid(m(proj)) * mix
    for b, n in enumerate(lens):
        want[b, n:] = 0
    _close(O.mask_fc_ref(proj, m.weight, mix, lens), want)


@pytest.mark.parametrize('k,act,pool', [(3, 'relu', False), (4, None, False), (3, 'relu', True), (3, 'lrelu', False)])
def test_conv2d_ref_is_nn_conv2d(k, act, pool):
    g = _g(4)
    m = torch.nn.Conv2d(5, 6, k, 1, 1).to(D)
    x = R.rnd(g, 2, 9, 7, 5).to(D)
    y = m(x.permute(0, 3, 1, 2))
    y = {None: lambda v: v, 'relu': torch.relu, 'lrelu': torch.nn.LeakyReLU(0.2)}[act](y)
    if pool:
        y = torch.nn.MaxPool2d(2, 2, ceil_mode=True)(y)
    _close(O.conv2d_ref(x, m.weight, m.bias, 1, 1, act, pool), y.permute(0, 2, 3, 1))
    got = O.conv2d_ref(x, m.weight, m.bias, 1, 1, act, pool, rows_out=[y.shape[2], 2])
    _close(got[0], y.permute(0, 2, 3, 1)[0])
    _close(got[1, :2], y.permute(0, 2, 3, 1)[1, :2])
    assert (got[1, 2:] == 0).all()


def test_conv_transpose2d_ref_is_nn_conv_transpose2d():
    g = _g(5)
    m = torch.nn.ConvTranspose2d(6, 4, 4, 2, 1).to(D)
    x = R.rnd(g, 2, 4, 3, 6).to(D)
    _close(O.conv_transpose2d_ref(x, m.weight, m.bias, 1), m(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))


@pytest.mark.parametrize('C', [6, 8])
def test_bn_lrelu_ref_is_nn_batchnorm2d(C):
    g = _g(6)
    m = torch.nn.BatchNorm2d(C).to(D).train()
    m.weight.data.copy_(1.0 + R.rnd(g, C, scale=0.2))
    m.bias.data.copy_(R.rnd(g, C, scale=0.1))
    x = R.rnd(g, 3, 5, 4, C).to(D)
    want = torch.nn.LeakyReLU(0.2)(m(x.permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    _close(O.bn_lrelu_ref(x, m.weight, m.bias, m.eps, 0.2), want)


@pytest.mark.parametrize('lens', [[5, 3, 1], [5, 5, 5]])
def test_bilstm_layer_ref_is_packed_nn_lstm(lens):
    g = _g(7)
    T, B, I, H = 5, 3, 12, 8
    m = torch.nn.LSTM(I, H, bidirectional=True).to(D)
    x = R.rnd(g, T, B, I).to(D)
    P = {}
    for d, suffix in (('f', ''), ('r', '_reverse')):
        for k, n in (('w_ih', 'weight_ih_l0'), ('w_hh', 'weight_hh_l0'), ('b_ih', 'bias_ih_l0'), ('b_hh', 'bias_hh_l0')):
            P['%s.%s' % (d, k)] = getattr(m, n + suffix)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lens), enforce_sorted=True)
    want = torch.nn.utils.rnn.pad_packed_sequence(m(packed)[0], total_length=T)[0]
    _close(O.bilstm_layer_ref(x, lens, P), want)


def test_embedding_ref_is_nn_embedding():
    m = torch.nn.Embedding(9, 6).to(D)
    ids = torch.tensor([3, 0, 3, 8, 5, 3, 0], dtype=torch.int32)
    _close(O.embedding_ref(m.weight, ids), m(ids.long()))


# ---------------------------------------------------------------------------------------------
# every row: the reference runs, owes a gradient to every parameter, and fp32 on the CPU is within a quarter of every bar
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', O.NAMES)
def test_rows_have_margin(name):
    row = O.BY_NAME[name]
    case = row.build()
    bars = row.bars(case)
    assert set(bars) == set(case['params']) | {'d_' + k for k in case['inputs']}
    assert set(row.cells) <= set(O.CELLS) and all(isinstance(v, str) and v for v in row.cells.values())
    groups = O.groups_of(row, case)
    assert groups and all(set(v) <= set(case['params']) and v for v in groups.values())
    for uses in (1, 2):
        w64, w32 = O.row_grads(row, case, torch.float64, uses), O.row_grads(row, case, torch.float32, uses)
        b = dict(bars, **{'d2_' + k: bars['d_' + k] for k in case['inputs']})
        O.margins(row, case, w64, w32, b)
        # the checker accepts the fp32 CPU run as a first write, and the same run on top of a prefill
        g0 = {k: torch.randn(v.shape, generator=_g(9)) * float(v.abs().max()) for k, v in w32.items()}
        assert O.check_protocol(w32, w64, w32, {}, None, b) == []
        assert O.check_protocol({k: g0[k] + v for k, v in w32.items()}, w64, w32, g0, None, b) == []


def test_second_use_differs_and_keeps_the_zeros():
    row = O.BY_NAME['linear-rows-T5B3-K12']
    case = row.build()
    two = O.second_use(case)
    assert ((two['dy'] == 0) == (case['dy'] == 0)).all() and not torch.equal(two['dy'], case['dy'])
    assert torch.equal(two['inputs']['x'], 0.5 * case['inputs']['x']) and two['params'] is case['params']


# ---------------------------------------------------------------------------------------------
# closure: no Function of ops.py that accumulates parameter gradients is left out of OPS
# ---------------------------------------------------------------------------------------------
def _functions():
    from robust_e2e_gan_amd import ops
    return ops, {n: c for n, c in vars(ops).items() if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == ops.__name__}


def _accumulates(ops, cls):
    """The class's source mentions accumulate(, or reaches a helper that does (the decoder's loops and upper layers, the padded linear
    backward, the fused bias gradient)."""
    src = inspect.getsource(cls)
    return 'accumulate(' in src or any(h + '(' in src for h in _helpers(ops))


@functools.lru_cache(maxsize=None)
def _helpers(ops):
    """The module-level functions of ops.py that accumulate, directly or through one another."""
    srcs = {n: inspect.getsource(f) for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and n != 'accumulate'}
    helpers = {n for n, s in srcs.items() if 'accumulate(' in s}
    for _ in range(3):                          # helpers that reach helpers
        helpers |= {n for n, s in srcs.items() if any(h + '(' in s for h in helpers)}
    return tuple(sorted(helpers))


def test_ops_table_is_closed(monkeypatch):
    ops, fns = _functions()
    assert {'_upper_backward', '_att_loop_backward'} <= set(vars(ops)), 'the helpers the closure follows have been renamed'
    with_rows = {r.fn for r in O.OPS}
    need = {n for n, c in fns.items() if _accumulates(ops, c)}
    assert {'DecoderLoopFn', 'DecoderUpperFn', 'LinearFn', 'Conv2dFn', 'BiLstmFn'} <= need
    assert need <= with_rows, 'Functions that accumulate parameter gradients without a row in refs64_ops.OPS: %s' % sorted(need - with_rows)
    rest = set(fns) - need
    assert rest == set(O.NO_PARAMETERS), 'NO_PARAMETERS is out of date: %s' % sorted(rest ^ set(O.NO_PARAMETERS))
    assert with_rows <= set(fns)
    # a row deleted: the closure fails
    monkeypatch.setattr(O, 'OPS', [r for r in O.OPS if r.fn != 'Linear2BiasFn'])
    assert not need <= {r.fn for r in O.OPS}


# ---------------------------------------------------------------------------------------------
# sensitivity: six fabricated results, each caught
# ---------------------------------------------------------------------------------------------
def _fabric():
    row = O.BY_NAME['linear-3x5x12-8-tanh']
    case = row.build()
    bars = row.bars(case)
    w64, w32 = O.row_grads(row, case, torch.float64), O.row_grads(row, case, torch.float32)
    g0 = {k: torch.randn(v.shape, generator=_g(10)) * float(v.abs().max()) for k, v in w32.items()}
    guard = torch.full((3 * O.GUARD,), O.SENTINEL)
    return row, case, bars, w64, w32, g0, guard


def test_check_protocol_accepts_the_honest_run():
    row, case, bars, w64, w32, g0, guard = _fabric()
    got = {k: g0[k] + w32[k] for k in w32}
    log = []
    assert O.check_protocol(got, w64, w32, g0, (guard, guard.clone()), bars, 'honest', log) == []
    assert len(log) == len(w64) and all(l.startswith('ERR honest') and 'fp32-cpu' in l and 'bar' in l for l in log)
    frozen = dict(w64, b=None)
    assert O.check_protocol(dict(got, b=g0['b'].clone()), frozen, w32, g0, None, bars) == []
    assert O.check_protocol(dict(w32, b=None), frozen, w32, {}, None, bars) == []


@pytest.mark.parametrize('mistake', ['overwrite', 'use dropped', 'frozen ulp', 'guard', 'unwritten', 'scaled', 'frozen written', 'missing'])
def test_check_protocol_catches(mistake):
    row, case, bars, w64, w32, g0, guard = _fabric()
    got = {k: g0[k] + w32[k] for k in w32}
    want64, after = dict(w64), guard.clone()
    if mistake == 'overwrite':                   # an overwrite where an accumulation was due
        got['W'] = w32['W'].clone()
    elif mistake == 'use dropped':               # one of two uses dropped
        want64 = O.row_grads(row, case, torch.float64, uses=2)
        want64 = {k: v for k, v in want64.items() if not k.startswith('d2_')}
    elif mistake == 'frozen ulp':                # a frozen buffer moved by one ulp
        want64['b'] = None
        moved = g0['b'].clone()
        moved[3] = torch.nextafter(moved[3], torch.tensor(float('inf')))
        got['b'] = moved
    elif mistake == 'guard':                     # a guard float changed
        after[O.GUARD] = 0.0
    elif mistake == 'unwritten':                 # one element left unwritten on a first write
        g0 = {}
        got = {k: v.clone() for k, v in w32.items()}
        got['W'][2, 5] = float('nan')
    elif mistake == 'scaled':                    # a gradient scaled by 2
        got['b'] = g0['b'] + 2 * w32['b']
    elif mistake == 'frozen written':
        want64['b'] = None
        g0 = {k: v for k, v in g0.items() if k != 'b'}
        got = {k: (w32[k] if k == 'b' else v) for k, v in got.items()}
    else:
        got['W'] = None
    bad = O.check_protocol(got, want64, w32, g0, (guard, after), bars)
    assert len(bad) == (2 if mistake == 'use dropped' else 1), bad          # (a dropped use shows on both parameters)
    hit = {'overwrite': 'W:', 'use dropped': 'W:', 'frozen ulp': 'b: excluded', 'guard': 'guard', 'unwritten': 'W:', 'scaled': 'b:', 'frozen written': 'b: excluded',
           'missing': 'W: no gradient'}[mistake]
    assert bad[0].startswith(hit), bad
