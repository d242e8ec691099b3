"""What tests/test_recog_cli_gpu.py recognises, built from a seed: a checkpoint from the enhancer and ASR parameters of
tests/golden/joint_tiny.npz with ``__graft_entry__._tiny_opt()``, a data directory of five utterances of F = 257 magnitudes (two speakers,
one utterance known to utt2spk / text_char only by the part of its id before ``__``), a 10-symbol dictionary with '<space>', the two CMVN
files and the LM of recog_lm_tiny.npz as a state dict.

FEATURE_SEED was chosen on the CPU with ``oracle.decode.recognize`` over the same parameters (``python tests/recog_fixture.py`` prints the
table): of the seeds 0 .. 19 it is the one whose smallest gap between adjacent n-best scores (beam 4, nbest 4, ctc-weight 0.3; with and
without the enhancer) is the largest, so that a 1e-5 difference between two paths of the search cannot reorder a list.  The test asserts the
gap on the device again."""
import os

import numpy as np
import torch

LENGTHS = [37, 29, 20, 33, 20]
UTTS = ['spkA-u0', 'spkA-u1', 'spkB-u2__cafe_5dB', 'spkB-u3', 'spkA-u4']
SYMBOLS = ['a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', '<space>']          # ids 1 .. 10; 0 = <blank>, 11 = <eos>
TEXTS = ['abca', 'dde', 'fghi', 'abc', 'iha']          # text_char is read character by character (audioparse.py:101-103): no '<space>' in a transcript
FEATURE_SEED = 5
BEAM = dict(beam_size=4, nbest=4, ctc_weight=0.3, penalty=0.0, maxlenratio=0.0, minlenratio=0.0)


def features(seed=None):
    rng = np.random.default_rng(FEATURE_SEED if seed is None else seed)
    return [(rng.random((T, 257)) * 2.0 + 0.01).astype(np.float32) for T in LENGTHS]


def spectrum_cmvn(feats):
    """[-mean; 1/std] of 10 log10(max(x, 1e-7)) over all frames, in float64: the data set's cmvn.npy, written so that it is not recomputed."""
    f = 10 * np.log10(np.maximum(np.concatenate(feats, 0).astype(np.float64), 1e-7))
    return np.stack([-f.mean(0), 1 / f.std(0)]).astype(np.float32)


def golden(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


def sub(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}


def targets():
    idx = {c: i + 1 for i, c in enumerate(SYMBOLS)}
    out = []
    for t in TEXTS:
        toks, k = [], 0
        while k < len(t):
            n = len('<space>') if t.startswith('<space>', k) else 1
            toks.append(idx[t[k:k + n]])
            k += n
        out.append(toks)
    return out


def build(root, golden_dir, seed=None):
    """Write everything under ``root``; returns a dict of paths and the in-memory pieces."""
    import __graft_entry__ as g
    from robust_e2e_gan_amd.data import kaldi_io
    fx = golden(golden_dir, 'joint_tiny.npz')
    opt = g._tiny_opt()
    exp = os.path.join(root, 'exp', 'tiny')
    data, dct = os.path.join(root, 'data'), os.path.join(root, 'dict')
    for d in (exp, data, dct):
        os.makedirs(d, exist_ok=True)
    torch.save({'opt': opt, 'enhance_state_dict': sub(fx, 'enh.'), 'asr_state_dict': sub(fx, 'asr.'), 'fbank_state_dict': None},
               os.path.join(exp, 'model.pth'))
    feats = features(seed)
    w = kaldi_io.ArkScpWriter(os.path.join(data, 'feats.ark'), False)
    for u, m in zip(UTTS, feats):
        w.add(u, m)
    w.close(os.path.join(data, 'feats.scp'))
    with open(os.path.join(data, 'utt2spk'), 'w') as f, open(os.path.join(data, 'text_char'), 'w') as t:
        for u, text in zip(UTTS, TEXTS):
            key = u.split('__')[0]
            f.write('%s %s\n' % (key, key.split('-')[0]))
            t.write('%s %s\n' % (key, text))
    with open(os.path.join(dct, 'train_units.txt'), 'w') as f:
        for k, s in enumerate(SYMBOLS):
            f.write('%s %d\n' % (s, k + 1))
    cmvn = spectrum_cmvn(feats)
    np.save(os.path.join(exp, 'cmvn.npy'), cmvn)
    np.save(os.path.join(exp, 'enhance_cmvn.npy'), fx['cmvn'])
    lm_path = os.path.join(root, 'rnnlm.model.best')
    torch.save(sub(golden(golden_dir, 'recog_lm_tiny.npz'), 'lm.'), lm_path)
    return dict(root=root, exp=exp, data=data, dict=dct, lm=lm_path, feats=feats, cmvn=cmvn, fbank_cmvn=fx['cmvn'], fx=fx, opt=opt,
                argv=['--recog-dir', data, '--dict_dir', dct, '--checkpoints_dir', os.path.join(root, 'exp'), '--name', 'tiny', '--works_dir', exp,
                      '--resume', 'model.pth', '--beam-size', '4', '--nbest', '4', '--ctc-weight', '0.3', '--verbose', '0'])


def oracle_gaps(golden_dir, seed, enhance=True):
    """Smallest gap between adjacent n-best scores over the five utterances, on the CPU."""
    from oracle import decode, nets
    fx = golden(golden_dir, 'joint_tiny.npz')
    enh, asr = sub(fx, 'enh.'), sub(fx, 'asr.')
    feats = features(seed)
    cm = torch.from_numpy(spectrum_cmvn(feats))
    W = torch.from_numpy(nets.mel_matrix(80)).float()
    gap = float('inf')
    for m in feats:
        x = torch.from_numpy(np.maximum(m, 1e-7))[None]
        if enhance:
            out = nets.enhance_forward(enh, x, (10 * torch.log10(x) + cm[0]) * cm[1], [x.shape[1]], 2)
            x = out[0] if isinstance(out, tuple) else out
        f = nets.fbank_forward(x, W, torch.from_numpy(fx['cmvn']))
        nb = decode.recognize(asr, f, 2, BEAM['beam_size'], BEAM['penalty'], BEAM['ctc_weight'], BEAM['maxlenratio'], BEAM['minlenratio'], BEAM['nbest'])
        s = [h['score'] for h in nb]
        gap = min([gap] + [float(a - b) for a, b in zip(s, s[1:])])
    return gap


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    gd = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    for seed in range(20):
        print(seed, '%.5f %.5f' % (oracle_gaps(gd, seed, True), oracle_gaps(gd, seed, False)))
