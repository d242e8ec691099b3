"""CPU-only: the host side of language-model training against tests/golden/lm_train_tiny.npz (written by the reference:
make_fixtures_lm_train.py) -- the batch iterator's output and counters, ``next_window`` against repeated ``__next__``, the command line's
options and defaults -- and what the trainer refuses."""
import argparse
import json
import os

import numpy as np
import pytest


@pytest.fixture(scope='module')
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'lm_train_tiny.npz')))


def _counters(it):
    return [it.iteration, it.epoch, int(it.is_new_epoch), it.epoch_detail, it.previous_epoch_detail]


def _state(it):
    return (it.iteration, it.epoch, it.is_new_epoch, it.epoch_detail, it.previous_epoch_detail, list(it.offsets))


def test_iterator_reproduces_the_reference(fx):
    from robust_e2e_gan_amd.data.lm_data_loader import ParallelSequentialIterator
    data = fx['iter.data']
    it = ParallelSequentialIterator(data, 4)
    assert it.epoch == 0 and it.is_new_epoch is False and it.iteration == 0 and it.previous_epoch_detail is None
    assert list(it.offsets) == fx['iter.offsets'].tolist() == [i * 23 // 4 for i in range(4)]
    for want, cnt in zip(fx['iter.batches'], fx['iter.counters']):
        got = it.__next__()
        assert isinstance(got, list) and len(got) == 4 and all(len(pair) == 2 for pair in got)
        assert np.array_equal(np.array(got), want)
        assert _counters(it) == cnt.tolist()
    assert it.epoch == 2 and len(fx['iter.batches']) == 12
    # repeat=False: stops once every token has been the current one, and starts over
    it = ParallelSequentialIterator(data, 4, repeat=False)
    n = 0
    with pytest.raises(StopIteration):
        while True:
            it.__next__()
            n += 1
    assert n == int(fx['iter.stop_after']) and it.iteration == int(fx['iter.iteration_after_stop']) and it.epoch == int(fx['iter.epoch_after_stop'])
    assert np.array_equal(np.array(it.__next__()), fx['iter.batches'][0])          # the next pass begins at the start


@pytest.mark.parametrize('n,batch,T', [(23, 4, 3), (23, 4, 1), (40, 4, 3), (7, 3, 5), (16, 4, 35)])
def test_next_window_is_repeated_next(n, batch, T):
    """(xs, ts) of a window = the stacked batches of T ``__next__`` calls, and the iterator is left in the same state; over several
    windows, across epoch boundaries and wrap-arounds of the corpus."""
    from robust_e2e_gan_amd.data.lm_data_loader import ParallelSequentialIterator
    data = (np.arange(n) * 5 % 11).astype(np.int32)
    a, b = ParallelSequentialIterator(data, batch), ParallelSequentialIterator(data, batch)
    for _ in range(6):
        xs, ts = a.next_window(T)
        want = np.stack([np.array(b.__next__()) for _ in range(T)])
        assert xs.dtype == np.int32 and ts.dtype == np.int32 and xs.shape == ts.shape == (T, batch)
        assert np.array_equal(xs, want[:, :, 0]) and np.array_equal(ts, want[:, :, 1])
        assert _state(a) == _state(b)
    assert a.epoch >= 1


def test_next_window_stops_where_next_would():
    from robust_e2e_gan_amd.data.lm_data_loader import ParallelSequentialIterator
    data = np.arange(23, dtype=np.int32)
    a, b = ParallelSequentialIterator(data, 4, repeat=False), ParallelSequentialIterator(data, 4, repeat=False)
    xs, ts = a.next_window(4)
    want = np.stack([np.array(b.__next__()) for _ in range(4)])
    assert np.array_equal(xs, want[:, :, 0]) and np.array_equal(ts, want[:, :, 1]) and _state(a) == _state(b)
    with pytest.raises(StopIteration):          # steps 5 and 6 exist, the 7th does not
        a.next_window(4)
    with pytest.raises(StopIteration):
        for _ in range(4):
            b.__next__()
    assert _state(a) == _state(b) and a.iteration == 0


def test_command_line_is_the_references(fx):
    from robust_e2e_gan_amd.lm_train import get_parser
    want = json.loads(str(fx['cli.table']))
    got = {}
    for act in get_parser()._actions:
        if act.dest != 'help':
            got[act.dest] = dict(default=act.default, flags=sorted(act.option_strings), type=getattr(act.type, '__name__', None), required=bool(act.required))
    assert got == want
    args = get_parser().parse_args(['--outdir', 'o', '--dict', 'd', '--train-label', 't', '--valid-label', 'v'])
    assert (args.batchsize, args.bproplen, args.epoch, args.gradclip, args.input_unit, args.unit, args.dropout_rate, args.lm_type, args.ngpu, args.seed) == \
        (2048, 35, 25, 5, 650, 650, 0.2, 'rnnlm', 0, 1)


def _args(**kw):
    base = dict(ngpu=1, outdir='/nonexistent', seed=1, train_label='/nonexistent/train', valid_label='/nonexistent/valid', lm_type='rnnlm', batchsize=4,
                bproplen=3, epoch=1, gradclip=5.0, input_unit=6, unit=10, dropout_rate=0.0, embed_init_file='', n_vocab=11,
                char_list_dict={str(i): i for i in range(11)})
    base.update(kw)
    return argparse.Namespace(**base)


def test_trainer_refuses_what_is_out_of_scope():
    """Before it opens a file: the FS-RNN LM, more than one GPU, training on the CPU."""
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model import lm
    for kw in (dict(lm_type='fsrnnlm'), dict(ngpu=2), dict(ngpu=0)):
        with pytest.raises(Re2eError):
            lm.train(_args(**kw))
    doc = lm.__doc__.split('Out of scope')[1]
    assert 'FS-RNN' in doc and 'several GPUs' in doc and 'CPU' in doc and 'n-gram' in doc and 'cold fusion' in doc
    assert 'lm_train.py' not in doc          # training itself has left the list
