"""python -m robust_e2e_gan_amd.joint_recog ...: enhancer -> filterbank -> beam search over a data set, then its error rates (recog.py)."""
from .recog import main as _main


def main(argv=None):
    return _main('joint', argv)


if __name__ == '__main__':
    main()
