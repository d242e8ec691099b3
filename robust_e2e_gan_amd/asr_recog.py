"""python -m robust_e2e_gan_amd.asr_recog ...: filterbank -> beam search over a data set, without the enhancer, then its error rates (recog.py)."""
from .recog import main as _main


def main(argv=None):
    return _main('asr', argv)


if __name__ == '__main__':
    main()
