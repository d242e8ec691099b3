"""Recognition flags (options/test_options.py:9-29, spellings and defaults as upstream) plus the ones the recognisers here add: they are
named so that they cannot collide with an upstream flag."""
from .base_options import BaseOptions


class TestOptions(BaseOptions):
    __test__ = False          # not a pytest class

    def initialize(self):
        BaseOptions.initialize(self)
        p = self.parser
        # task related
        p.add_argument('--recog-dir', type=str, help='data directory to recognise (feats.scp, utt2spk, text_char | text_word)')
        p.add_argument('--enhance-dir', type=str, help='accepted for command-line compatibility')
        p.add_argument('--enhance-out-dir', type=str, help='accepted for command-line compatibility')
        p.add_argument('--recog-label', type=str, help='accepted for command-line compatibility')
        p.add_argument('--recog-json', type=str, help='accepted for command-line compatibility')
        p.add_argument('--result-label', type=str, help='result JSON to write')
        p.add_argument('--nj', type=int, default=1, help='accepted and ignored: one process decodes the set')
        # search related
        p.add_argument('--nbest', type=int, default=1, help='Output N-best hypotheses')
        p.add_argument('--beam-size', type=int, default=1, help='Beam size')
        p.add_argument('--penalty', default=0.0, type=float, help='Insertion penalty')
        p.add_argument('--maxlenratio', default=0.0, type=float, help='Input length ratio to obtain max output length; 0.0: end detection')
        p.add_argument('--minlenratio', default=0.0, type=float, help='Input length ratio to obtain min output length')
        p.add_argument('--ctc-weight', default=0.0, type=float, help='CTC weight in joint decoding')
        p.add_argument('--fstlm-path', type=str, help='refused: FST / n-gram LMs are out of scope')
        p.add_argument('--nn-char-map-file', type=str, help='accepted for command-line compatibility')
        # ---- not upstream -----------------------------------------------------------------------------------------------------------
        p.add_argument('--recog-batch', type=int, default=16, help='utterances per search (1: the reference\'s loop, one recognize per utterance)')
        p.add_argument('--fbank_cmvn', type=str, default=None, help='CMVN of the filterbank features (.npy); default: exp_path/fbank_cmvn.npy, '
                                                                    'then exp_path/enhance_cmvn.npy')
        p.add_argument('--score', dest='score', action='store_true', default=True, help='score the result on the device (default)')
        p.add_argument('--no-score', dest='score', action='store_false', help='write the result JSON only')
        p.add_argument('--score-costs', type=str, default='4,3,3', help='alignment costs S,I,D (4,3,3: the NIST weights; 1,1,1: Levenshtein)')
        p.add_argument('--score-dir', type=str, default=None, help='where ref.trn, hyp.trn, score.json and result.txt go; default: beside --result-label')
        # the FS-RNN LM's shape (lm_train's flags and defaults)
        p.add_argument('--fast_layers', type=int, default=2)
        p.add_argument('--fast_cell_size', type=int, default=650)
        p.add_argument('--slow_cell_size', type=int, default=650)
        p.add_argument('--zoneout_keep_h', type=float, default=0.9)
        p.add_argument('--zoneout_keep_c', type=float, default=0.5)

    def parse(self, argv=None, save=False):
        """As BaseOptions.parse, but opt.txt is written only when asked for: recognising must not touch the experiment directory."""
        return BaseOptions.parse(self, argv, save)
