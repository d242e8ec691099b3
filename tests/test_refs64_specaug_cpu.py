"""CPU-only: the references of tests/refs64_specaug.py agree with each other (the integer restatement of include/re2e.h's contract against
``F.interpolate`` itself, forward and -- as a gather over inverted tap ranges -- backward), the inputs of the GPU tests leave the bars their
margin, and the host side of SpecAugment: the configuration string, the plan draws and their random stream, the trainers' step counter."""
import argparse

import numpy as np
import pytest
import torch

import refs64_specaug as RS

CASES = RS.cases()
_REF = {}


def ref_of(name):
    """(x, dy, clamped plan, y64, dx64) of a case, computed once per session and shared (tests/test_specaug_kernels_gpu.py reads it too)."""
    if name not in _REF:
        c = CASES[name]
        x, dy, plan = RS.case_tensors(c)
        y, dx = RS.specaug_ref(x, plan, c['nF'], c['nT'], dy)
        _REF[name] = (x, dy, plan, y, dx)
    return _REF[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_equals_interpolate(name):
    c = CASES[name]
    x, dy, plan, y, dx = ref_of(name)
    y2, dx2 = RS.specaug_restated(x, plan, c['nF'], c['nT'], dy)
    assert RS.rel_err(y2, y) <= 1e-10 and RS.rel_err(dx2, dx) <= 1e-10, (RS.rel_err(y2, y), RS.rel_err(dx2, dx))
    R, Tp, F = c['shape']
    for r in range(R):
        T = int(plan[r, 0])
        assert torch.equal(y[r, T:], x[r, T:].double()) and torch.equal(dx[r, T:], dy[r, T:].double())      # the padding passes through
    if c['exact']:
        assert torch.equal(y, x.double()) and torch.equal(y2, x.double())
    if name == 'full_F':
        for r in range(R):
            T = int(plan[r, 0])
            assert not y[r, :T].any() and not dx[r, :T].any()


@pytest.mark.parametrize('name', sorted(CASES))
def test_margins(name):
    """The preconditions of the GPU bars: the fp32 CPU run of the reference stays within a quarter of each."""
    c = CASES[name]
    x, dy, plan, y, dx = ref_of(name)
    y32, dx32 = RS.specaug_ref(x, plan, c['nF'], c['nT'], dy, dtype=torch.float32)
    RS.margin_ok(name + ' y', y32, y, RS.BAR_FBANK_OUT)
    RS.margin_ok(name + ' dx', dx32, dx, RS.BAR_FBANK_GRAD)


def test_tap_ranges_are_the_hit_sets():
    """``taps_range`` (i0(t) inverted in integers) names exactly the output frames whose clamped taps hit a source frame, as one contiguous run:
    squeezes down to 1 frame, stretches up to 2x and beyond."""
    for n_in in list(range(1, 14)) + [40]:
        for n_out in list(range(1, 27)) + [79, 81]:
            if n_in == n_out:
                continue
            for j in range(n_in):
                lo, hi = RS.taps_range(n_in, n_out, j)
                assert RS.full_jacobian_hits(n_in, n_out, j) == list(range(lo, hi)), (n_in, n_out, j, lo, hi)


def test_restatement_at_wide_size_pairs():
    """The size pairs of the issue's own check, 80 -> 1 and 80 -> 159 among them, forward only, one segment each."""
    g = torch.Generator().manual_seed(3)
    for n_in, n_out in ((1, 1), (1, 7), (2, 3), (5, 1), (80, 1), (80, 159), (80, 81), (81, 80), (400, 395), (7, 13)):
        x = torch.randn(n_in, 3, generator=g, dtype=torch.float64)
        ref = RS._resize(x, n_out)
        got = torch.stack([sum(w * x[i] for i, w in zip(*RS.taps(n_in, n_out, t))) for t in range(n_out)], 0)
        assert (got - ref).abs().max().item() <= 1e-10 * max(1.0, ref.abs().max().item()), (n_in, n_out)


def test_clamp_plan():
    c = CASES['clamped']
    R, Tp, F = c['shape']
    p = RS.clamp_plan(c['plan'], Tp, F, c['nF'], c['nT'])
    assert p.tolist() == [[200, 199, 1, 0, 5, 150, 50], [0, 0, 0, 8, 0, 0, 0], [60, 59, 59, 6, 2, 60, 0], [200, 1, 199, 2, 0, 0, 30]]
    for name, k in CASES.items():
        if not k['clamp']:
            assert np.array_equal(RS.clamp_plan(k['plan'], k['shape'][1], k['shape'][2], k['nF'], k['nT']), k['plan']), name


# ---------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------
def test_parse():
    from robust_e2e_gan_amd.data import spec_augment as sa
    cfg = sa.parse('5,30,2,40,2')
    assert tuple(cfg) == (5, 30, 2, 40, 2) and (cfg.W, cfg.F, cfg.nF, cfg.T, cfg.nT) == (5, 30, 2, 40, 2)
    assert sa.parse(' 0, 0,0 ,0,0 ') == sa.Config(0, 0, 0, 0, 0)
    assert sa.parse(None) is None and sa.parse('') is None and sa.parse(cfg) is cfg
    for bad, word in (('5,30,2,40', 'five'), ('5,30,2,40,2,1', 'five'), ('5,x,2,40,2', 'F (widest'), ('5,30,2,4.5,2', 'T (widest'),
                      ('-1,30,2,40,2', 'W (time-warp'), ('5,30,9,40,2', 'at most'), ('5,30,2,40,9', 'at most'), ('a', 'five')):
        with pytest.raises(ValueError) as e:
            sa.parse(bad)
        assert word in str(e.value) and 'spec_augment' in str(e.value), (bad, str(e.value))


def test_draw_plan_is_a_function_of_its_key():
    from robust_e2e_gan_amd.data import spec_augment as sa
    lens = [100, 57, 11, 10, 1]
    a = sa.draw_plan(7, 3, 0, lens, 80, '5,30,2,40,2')
    np.random.seed(99)
    np.random.default_rng(5).integers(10)
    b = sa.draw_plan(7, 3, 0, lens, 80, sa.parse('5,30,2,40,2'))
    assert a.dtype == np.int32 and a.shape == (5, 11) and np.array_equal(a, b)
    for other in ((8, 3, 0), (7, 4, 0), (7, 3, 1)):
        assert not np.array_equal(a, sa.draw_plan(*other, lens, 80, '5,30,2,40,2')), other
    # the stream is (seed, step, rank, 3)
    rng = np.random.default_rng([7, 3, 0, 3])
    c = int(rng.integers(5, 95))
    assert (int(a[0, 1]), int(a[0, 2])) == (c, int(rng.integers(c - 4, c + 6)))
    ident = sa.identity_plan(lens, '5,30,2,40,2')
    assert ident[:, 0].tolist() == lens and not ident[:, 1:].any()


def test_draw_plan_ranges():
    """200 draws at T = 100, W = 5: every value within its range, every row warps, and the validation of ops.spec_augment accepts them;
    rows with T_r <= 2W never warp."""
    from robust_e2e_gan_amd.data import spec_augment as sa
    cfg = sa.parse('5,30,2,40,2')
    seen_c, seen_d = set(), set()
    for step in range(200):
        p = sa.draw_plan(1, step, 0, [100, 10, 9, 1], 80, cfg)
        T, c, w = p[0, :3].tolist()
        assert T == 100 and 5 <= c <= 94 and c - 4 <= w <= c + 5, p[0]
        seen_c.add(c)
        seen_d.add(w - c)
        for r in range(4):
            T = int(p[r, 0])
            for k in range(2):
                f0, f = p[r, 3 + 2 * k:5 + 2 * k].tolist()
                assert 0 <= f <= 30 and 0 <= f0 <= 80 - f
                t0, t = p[r, 7 + 2 * k:9 + 2 * k].tolist()
                assert 0 <= t <= min(40, T) and 0 <= t0 <= T - t
        assert not p[1:, 1:3].any()                        # T_r = 10 = 2W, 9, 1: no warp
        q, nT = sa.validate_plan(p, 100, 80, 2)
        assert nT == 2 and np.array_equal(q, p)
        assert np.array_equal(RS.clamp_plan(p, 100, 80, 2, 2), p)
    assert min(seen_c) <= 10 and max(seen_c) >= 89 and seen_d == set(range(-4, 6))
    assert sa.draw_plan(1, 0, 0, [11], 80, cfg)[0, 1] == 5          # T_r = 2W + 1: the only centre
    assert not sa.draw_plan(1, 0, 0, [100], 80, '0,30,2,40,2')[0, 1:3].any()


def test_validate_plan_refuses_by_name():
    from robust_e2e_gan_amd.data import spec_augment as sa
    ok = [[30, 12, 15, 2, 3, 20, 10]]
    sa.validate_plan(ok, 30, 8, 1)
    for name, c in CASES.items():
        if not c['clamp']:
            sa.validate_plan(c['plan'], c['shape'][1], c['shape'][2], c['nF'])
    for row, word in (([31, 0, 0, 0, 0, 0, 0], 'T_r'), ([30, 12, 30, 0, 0, 0, 0], 'warp window'), ([30, 29, 29, 0, 0, 0, 0], 'warp window'),
                      ([30, -1, 3, 0, 0, 0, 0], 'warp window'), ([30, 0, 0, 7, 2, 0, 0], 'frequency mask'), ([30, 0, 0, 0, -1, 0, 0], 'frequency mask'),
                      ([30, 0, 0, 0, 0, 25, 6], 'time mask'), ([30, 0, 0, 0, 0, -1, 0], 'time mask')):
        with pytest.raises(ValueError) as e:
            sa.validate_plan([row], 30, 8, 1)
        assert word in str(e.value), (row, str(e.value))
    with pytest.raises(ValueError):
        sa.validate_plan([[30, 0, 0, 0]], 30, 8, 0)
    with pytest.raises(ValueError):
        sa.validate_plan(ok, 30, 8, 3)


def test_other_random_streams_are_untouched():
    """The augmentation draws on stream 3 of its own key: the mixture, RIR and speed draws return what they return without it."""
    from robust_e2e_gan_amd.data import spec_augment as sa
    from robust_e2e_gan_amd.data import wav_dataset as wd
    want = [(wd.draw_mixture(5, e, i, [4000, 9000], 3000), wd.draw_reverb(5, e, i, 7, 0.5), wd.draw_speed(5, e, i, 3)) for e in range(2) for i in range(6)]
    got = []
    for e in range(2):
        for i in range(6):
            sa.draw_plan(5, e, i, [100, 80], 80, '5,30,2,40,2')
            got.append((wd.draw_mixture(5, e, i, [4000, 9000], 3000), wd.draw_reverb(5, e, i, 7, 0.5), wd.draw_speed(5, e, i, 3)))
    assert got == want
    # and they are the draws of the generators the datasets have always seeded
    rng = np.random.default_rng([5, 1, 2])
    ni = int(rng.integers(2))
    assert wd.draw_mixture(5, 1, 2, [4000, 9000], 3000)[0] == ni
    assert wd.draw_speed(5, 1, 2, 3) == int(np.random.default_rng([5, 1, 2, 2]).integers(3))


def _tiny(spec=None):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), 'spec_augment': spec, 'seed': 11})


def test_trainer_counters_survive_state_and_uncount():
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import E2E, ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    from robust_e2e_gan_amd.trainers import AsrTrainer
    opt = _tiny('2,4,1,5,1')
    lens = torch.IntTensor([37, 29, 20])
    mk = {'joint': lambda o: JointTrainer(o, EnhanceModel(o), FbankModel(o), ShareE2E(o), GANModel(o)), 'asr': lambda o: AsrTrainer(o, E2E(o))}
    draw = {'joint': lambda tr: tr._draw_aug(lens), 'asr': lambda tr: tr._draw_aug(lens, 80)}
    for kind in ('joint', 'asr'):
        tr = mk[kind](opt)
        assert tr.aug_step == 0 and tuple(tr.spec_augment) == (2, 4, 1, 5, 1)
        p0, p1 = draw[kind](tr), draw[kind](tr)
        assert tr.aug_step == 2 and p0.nF == 1 and p0.rows.shape == (3, 7) and not np.array_equal(p0.rows, p1.rows)
        assert p0.rows[:, 0].tolist() == [37, 29, 20]
        tr._uncount_step()
        assert tr.aug_step == 1 and np.array_equal(draw[kind](tr).rows, p1.rows)      # the step that is run again sees its plan
        st = tr.state(0, 0) if kind == 'joint' else tr.state()
        assert st['spec_augment_step'] == 2
        p2 = draw[kind](tr)
        other = mk[kind](opt)
        other.load_state(st)
        assert other.aug_step == 2 and np.array_equal(draw[kind](other).rows, p2.rows)
        # without the option: no plan, nothing counted, nothing taken back
        plain = mk[kind](_tiny(None))
        assert plain.spec_augment is None and draw[kind](plain) is None and plain.aug_step == 0
        plain._uncount_step()
        assert plain.aug_step == 0
        assert 'spec_augment_step' not in (plain.state(0, 0) if kind == 'joint' else plain.state())      # the checkpoint keys are what they were
        plain.load_state({k: v for k, v in st.items() if k != 'spec_augment_step'})
        assert plain.aug_step == 0


def test_recovering_an_aborted_step_repeats_its_own_plan(monkeypatch):
    """JointTrainer.recover_aborted_step with a stubbed ``step`` (host only): the repeat of an aborted step draws the plan the aborted attempt drew,
    whether or not a held step was enqueued behind it, and leaves the counter where ``fit`` expects it -- every enqueued step counted, so that
    ``_uncount_step`` + the held step's re-run draws the held step's own plan."""
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    opt = _tiny('2,4,1,5,1')
    lens = torch.IntTensor([37, 29, 20])
    tr = JointTrainer(opt, EnhanceModel(opt), FbankModel(opt), ShareE2E(opt), GANModel(opt))
    drawn = []

    def step(data, rate, cmvn):
        drawn.append((tr.aug_step, tr._draw_aug(lens).rows.copy()))
        return {'train/loss': torch.tensor(1.0), 'grad_norm': torch.tensor(1.0), 'aborts': torch.tensor(0.0)}
    monkeypatch.setattr(tr, 'step', step)
    monkeypatch.setattr(tr, '_acknowledge_aborts', lambda: None)
    entry = lambda: (None, 0.0, None, tr._bn_snapshot(), tr._rng_snapshot(), tr.aug_step)
    for _ in range(3):                                     # steps 0, 1, 2 went through
        tr.step(None, 0.0, None)
    # step 3 aborts with step 4 held behind it
    e3 = entry()
    tr.step(None, 0.0, None)
    tr.step(None, 0.0, None)
    assert tr.aug_step == 5
    vals = tr.recover_aborted_step(e3, 1)
    assert vals == {'train/loss': 1.0} and tr.recovered_steps == 1
    assert drawn[-1][0] == 3 and np.array_equal(drawn[-1][1], drawn[3][1])      # the repeat saw step 3's plan
    assert tr.aug_step == 5
    tr._uncount_step()                                     # fit(): the held step is run again
    tr.step(None, 0.0, None)
    assert drawn[-1][0] == 4 and np.array_equal(drawn[-1][1], drawn[4][1]) and tr.aug_step == 5
    # the last step of a run aborts: nothing behind it
    e5 = entry()
    tr.step(None, 0.0, None)
    tr.recover_aborted_step(e5, 2)
    assert drawn[-1][0] == 5 and np.array_equal(drawn[-1][1], drawn[-2][1]) and tr.aug_step == 6
    # nothing gave up: nothing is repeated, nothing taken back
    n = len(drawn)
    assert tr.recover_aborted_step(e5, 0) is None and len(drawn) == n and tr.aug_step == 6
    # an entry of the older, five-element form still repeats, on the count taken back
    e6 = entry()[:5]
    tr.step(None, 0.0, None)
    tr.recover_aborted_step(e6, 1)
    assert drawn[-1][0] == 6 and tr.aug_step == 7


def test_cli_takes_the_option():
    from robust_e2e_gan_amd.options.train_options import TrainOptions
    o = TrainOptions().parse(['--gpu_ids', '-1', '--spec_augment', '5,30,2,40,2'], save=False)
    assert o.spec_augment == '5,30,2,40,2'
    assert TrainOptions().parse(['--gpu_ids', '-1'], save=False).spec_augment is None
