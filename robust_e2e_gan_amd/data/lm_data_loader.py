"""Batches for training the language model on one long token sequence (the iterator lm.train reads, data/lm_data_loader.py upstream).

Row i of a batch walks the corpus from offset ``i * len // batch_size``; one step yields, per row, the token at the current position and
the one after it (input and target), positions wrapping at the end of the corpus.  ``next_window(T)`` gives T consecutive steps at once
as two (T, B) arrays built by index arithmetic -- the window one truncated-BPTT pass consumes (model/lm.py forward_seq)."""
import numpy as np


class ParallelSequentialIterator(object):
    def __init__(self, dataset, batch_size, repeat=True):
        self.dataset = dataset
        self.batch_size = batch_size
        self.repeat = repeat
        self.epoch = 0                  # completed sweeps: steps * batch_size // len
        self.is_new_epoch = False       # the last step completed a sweep
        self.iteration = 0              # steps taken (not parameter updates)
        n = len(dataset)
        self.offsets = [i * n // batch_size for i in range(batch_size)]
        self._previous_epoch_detail = -1.

    def __iter__(self):
        return self

    @property
    def epoch_detail(self):
        return self.iteration * self.batch_size / len(self.dataset)

    @property
    def previous_epoch_detail(self):
        return None if self._previous_epoch_detail < 0 else self._previous_epoch_detail

    def _exhausted(self):
        return not self.repeat and self.iteration * self.batch_size >= len(self.dataset)

    def _advance(self):
        self._previous_epoch_detail = self.epoch_detail
        self.iteration += 1
        epoch = self.iteration * self.batch_size // len(self.dataset)
        self.is_new_epoch = self.epoch < epoch
        if self.is_new_epoch:
            self.epoch = epoch

    def get_words(self):
        n = len(self.dataset)
        return [self.dataset[(off + self.iteration) % n] for off in self.offsets]

    def __next__(self):
        """A list of batch_size (current token, next token) pairs.  With repeat=False: StopIteration once every token has been the
        current one, and the iterator starts over."""
        if self._exhausted():
            self.iteration = 0
            raise StopIteration
        cur = self.get_words()
        self._advance()
        return list(zip(cur, self.get_words()))

    next = __next__

    def next_window(self, T):
        """(xs, ts), both (T, B) int32: the inputs and targets of the next T steps -- equal to T calls of ``__next__`` stacked, and
        leaving the iterator in the same state.  With repeat=False a window that would run past the stop raises StopIteration at the
        step where ``__next__`` would, the steps before it taken."""
        data = np.asarray(self.dataset)
        n, off = len(data), np.asarray(self.offsets, np.int64)
        for t in range(T):
            if self.repeat:
                break
            if (self.iteration + t) * self.batch_size >= n:
                for _ in range(t):
                    self._advance()
                self.iteration = 0
                raise StopIteration
        pos = off[None, :] + (self.iteration + np.arange(T, dtype=np.int64))[:, None]
        xs, ts = data[pos % n].astype(np.int32), data[(pos + 1) % n].astype(np.int32)
        for _ in range(T):
            self._advance()
        return xs, ts
