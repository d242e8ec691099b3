"""CPU-only: the decode-side language-model surface (robust_e2e_gan_amd/model/lm.py) imports without a GPU, carries the
reference's state_dict names and shapes (tests/golden/recog_lm_tiny.npz holds a state dict the reference wrote), initialises as
upstream does and refuses what is out of scope."""
import os

import numpy as np
import pytest
import torch


def _lm_arrays(golden_dir):
    fx = np.load(os.path.join(golden_dir, 'recog_lm_tiny.npz'))
    return {k[len('lm.'):]: fx[k] for k in fx.files if k.startswith('lm.')}


def test_state_dict_matches_reference_checkpoint(golden_dir):
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    ref = _lm_arrays(golden_dir)
    lm = ClassifierWithState(RNNLM(12, 6, 10))
    sd = lm.state_dict()
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    assert set(sd) == {'predictor.' + k for k in ('embed.weight', 'l1.weight_ih', 'l1.weight_hh', 'l1.bias_ih', 'l1.bias_hh', 'l2.weight_ih',
                                                   'l2.weight_hh', 'l2.bias_ih', 'l2.bias_hh', 'lo.weight', 'lo.bias')}
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, (k, tuple(v.shape), ref[k].shape)
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes['predictor.embed.weight'] == (12, 6) and shapes['predictor.l1.weight_ih'] == (40, 6)
    assert shapes['predictor.l1.weight_hh'] == shapes['predictor.l2.weight_ih'] == shapes['predictor.l2.weight_hh'] == (40, 10)
    assert shapes['predictor.lo.weight'] == (12, 10) and shapes['predictor.lo.bias'] == (12,)
    res = lm.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in lm.state_dict().items():
        assert np.array_equal(v.numpy(), ref[k]), k


def test_fresh_initialisation_is_uniform_pm_0p1():
    from robust_e2e_gan_amd.model.lm import RNNLM
    torch.manual_seed(3)
    lm = RNNLM(50, 7, 9)
    for k, v in lm.state_dict().items():
        assert v.abs().max().item() <= 0.1, k
    assert lm.embed.weight.abs().max().item() > 0.09          # spread over the interval, not collapsed at zero
    emb = np.linspace(-1, 1, 50 * 7, dtype=np.float32).reshape(50, 7)
    assert np.array_equal(RNNLM(50, 7, 9, embed_vecs_init=emb).embed.weight.detach().numpy(), emb)


def test_training_side_is_refused():
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    lm = ClassifierWithState(RNNLM(12, 6, 10))
    assert lm.training
    with pytest.raises(Re2eError):
        lm.predictor(None, torch.tensor([1, 2]))               # training mode: dropout would be live, the LM is decode-only here
    with pytest.raises(Re2eError):
        lm(None, torch.tensor([1, 2]), torch.tensor([2, 3]))    # the training loss
    lm.eval()
    with pytest.raises(Re2eError):
        lm.predict(None, torch.tensor([1, 2]))                  # parameters on the CPU: no fallback
