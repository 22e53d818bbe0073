"""Device buffers with sentinel guards for the hook tests (tests only; needs a GPU): an operand or output of `shape` (rows of pitch
`ld` >= shape[-1]) sits between two runs of GUARD sentinel elements, and the pad columns between its rows hold the sentinel too, so
that a store outside the documented outputs shows."""
import ctypes as C

import numpy as np
import torch

GUARD = 64             # elements of sentinel on either side (256 bytes: the body stays 16-byte aligned)
SENTINEL = {np.dtype(np.float32): -12345.0, np.dtype(np.int32): -777}


class Guarded:
    def __init__(self, *shape, ld=None, dtype=np.float32, init=None):
        self.shape, self.ld, self.dtype = shape, ld or shape[-1], np.dtype(dtype)
        self.rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        self.sent = SENTINEL[self.dtype]
        host = np.full(2 * GUARD + self.rows * self.ld, self.sent, dtype=self.dtype)
        if init is not None:
            host[GUARD:-GUARD].reshape(self.rows, self.ld)[:, :shape[-1]] = np.asarray(init, dtype=self.dtype).reshape(self.rows, shape[-1])
        self.buf = torch.from_numpy(host).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.dtype.itemsize * GUARD)

    def raw(self):
        """the whole body (rows * ld elements), after checking the guards around it"""
        a = self.buf.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[-GUARD:] == self.sent).all(), "elements around the buffer were written"
        return a[GUARD:-GUARD].copy()

    def read(self, written_cols=None):
        """the written columns as an array of `shape`; everything else in the buffer must still be the sentinel"""
        body = self.raw().reshape(self.rows, self.ld)
        n = written_cols or self.shape[-1]
        assert (body[:, n:] == self.sent).all(), "columns between the rows of a strided buffer were written"
        return body[:, :n].reshape(self.shape[:-1] + (n,)).copy()

    def untouched(self):
        return bool((self.buf == self.sent).all())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
