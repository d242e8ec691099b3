"""Train the recurrent language model the beam search decodes with (mirror of lm_train.py): the reference's flags and defaults, then
model/lm.py train() (--lm-type rnnlm) or model/fsrnn.py train() (--lm-type fsrnnlm).  python -m robust_e2e_gan_amd.lm_train --ngpu 1 --outdir exp/lm --dict data/dict.txt --train-label .. --valid-label .."""
import argparse
import logging
import random

import numpy as np


def get_parser():
    parser = argparse.ArgumentParser()
    # general configuration
    parser.add_argument('--ngpu', default=0, type=int, help='GPUs to train on (1; 0 and more than 1 are refused)')
    parser.add_argument('--outdir', type=str, required=True, help='where rnnlm.model.<epoch>, rnnlm.state.<epoch> and rnnlm.model.best go')
    parser.add_argument('--debugmode', default=1, type=int, help='accepted for command-line compatibility')
    parser.add_argument('--dict', type=str, required=True, help='token list, one token (and anything after a blank) per line')
    parser.add_argument('--seed', default=1, type=int, help='seed of the parameter initialisation and the dropout masks')
    parser.add_argument('--minibatches', '-N', type=int, default='-1', help='accepted for command-line compatibility')
    parser.add_argument('--verbose', '-V', default=0, type=int, help='> 0: log at INFO level')
    parser.add_argument('--embed-init-file', type=str, default='', help='Initial embedding vectors, one "token v1 v2 .." line each')
    # task related
    parser.add_argument('--train-label', type=str, required=True, help='training text: one line of blank-separated tokens')
    parser.add_argument('--valid-label', type=str, required=True, help='validation text: one line of blank-separated tokens')
    parser.add_argument('--lm-type', type=str, default='rnnlm', help='rnnlm or fsrnnlm')
    # LSTMLM training configuration
    parser.add_argument('--batchsize', '-b', type=int, default=2048, help='rows of a batch: parallel positions in the corpus')
    parser.add_argument('--bproplen', '-l', type=int, default=35, help='steps per truncated-BPTT window')
    parser.add_argument('--epoch', '-e', type=int, default=25, help='sweeps over the training text')
    parser.add_argument('--gradclip', '-c', type=float, default=5, help='global gradient-norm threshold')
    parser.add_argument('--input-unit', type=int, default=650, help='width of the embedding')
    parser.add_argument('--unit', '-u', type=int, default=650, help='LSTM units per layer')
    parser.add_argument('--dropout-rate', type=float, default=0.2, help='rate of the three dropouts')
    # FSLSTMLM training configuration (--lm-type fsrnnlm)
    parser.add_argument('--fast_cell_size', type=int, default=650, help='FS-RNN only')
    parser.add_argument('--slow_cell_size', type=int, default=650, help='FS-RNN only')
    parser.add_argument('--fast_layers', type=int, default=2, help='FS-RNN only')
    parser.add_argument('--zoneout_keep_c', type=float, default=0.5, help='FS-RNN only')
    parser.add_argument('--zoneout_keep_h', type=float, default=0.9, help='FS-RNN only')
    return parser


def main(argv=None):
    args = get_parser().parse_args(argv)
    fmt = '%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s'
    logging.basicConfig(level=logging.INFO if args.verbose > 0 else logging.WARN, format=fmt)
    random.seed(args.seed)
    np.random.seed(args.seed)
    with open(args.dict, 'rb') as f:
        char_list = [entry.decode('utf-8').split(' ')[0] for entry in f.readlines()]
    char_list.insert(0, '<blank>')
    char_list.append('<eos>')
    args.char_list_dict = {x: i for i, x in enumerate(char_list)}
    args.n_vocab = len(char_list)
    if args.lm_type == 'fsrnnlm':
        from .model import fsrnn
        return fsrnn.train(args)
    from .model import lm
    return lm.train(args)


if __name__ == '__main__':
    main()
