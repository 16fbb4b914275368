"""A row that is +0.0 except in a few windows, for the window forms of the models (tests/*_model.py): what a test of a row of more
than 2^32 elements can hold on the host.  Positions are Python integers or int64 arrays; nothing here is ever as long as the row."""
import numpy as np

F32 = np.float32


class SparseMask:
    """n bytes of a frame mask as stretches that tile [0, n): pieces = [(lo, hi, v)], ascending, v an integer (every byte of the
    stretch holds it) or a uint8 array of hi - lo bytes.  A non-zero byte keeps its frame"""

    def __init__(self, n, pieces):
        self.n = int(n)
        self.pieces = []
        at = 0
        for lo, hi, v in pieces:
            assert lo == at and hi > lo, (at, lo, hi)
            if not isinstance(v, (int, np.integer)):
                v = np.ascontiguousarray(v, np.uint8).reshape(-1)
                assert len(v) == hi - lo
            else:
                assert 0 <= int(v) < 256
            self.pieces.append((int(lo), int(hi), v))
            at = hi
        assert at == self.n, (at, self.n)

    @classmethod
    def of_dense(cls, m, ranges):
        """the stretches of a dense uint8 [n] mask that is constant between the windows `ranges` = [(lo, hi)]"""
        m = np.asarray(m, np.uint8)
        pieces, at = [], 0
        for lo, hi in list(ranges) + [(len(m), len(m))]:
            if lo > at:
                assert (m[at:lo] == m[at]).all(), "the dense mask is not constant outside its windows"
                pieces.append((at, lo, int(m[at])))
            if hi > lo:
                pieces.append((lo, hi, m[lo:hi]))
            at = max(at, hi)
        return cls(len(m), pieces)

    def kept(self, lo, hi, v):
        """kept frames of one stretch, a Python integer"""
        return (hi - lo if v else 0) if isinstance(v, (int, np.integer)) else int(np.count_nonzero(v))

    def count(self):
        """K: the kept frames of the whole mask, a Python integer"""
        return sum(self.kept(*p) for p in self.pieces)

    def places(self, a, b):
        """int64 [min(b, K) - a]: the frames that the kept frames number a, a + 1, .. are (Python integers per stretch)"""
        out, before = [], 0
        for lo, hi, v in self.pieces:
            k = self.kept(lo, hi, v)
            j0, j1 = max(a, before), min(b, before + k)
            if j1 > j0:
                if isinstance(v, (int, np.integer)):
                    out.append(np.arange(lo + j0 - before, lo + j1 - before, dtype=np.int64))
                else:
                    out.append(lo + np.flatnonzero(v)[j0 - before:j1 - before].astype(np.int64))
            before += k
        return np.concatenate(out) if out else np.zeros(0, np.int64)

    def clipped(self, n):
        """the mask cut to its first n bytes"""
        assert 0 <= n <= self.n
        return SparseMask(n, [(lo, min(hi, n), v if isinstance(v, (int, np.integer)) else v[:min(hi, n) - lo]) for lo, hi, v in self.pieces if lo < n])


class SparseRow:
    """lines x n float32, +0.0 outside the windows.  wins: [(offset, float32 [lines][length])], ascending, disjoint, inside
    [0, n)"""

    def __init__(self, n, wins, lines=1):
        self.n, self.lines = int(n), int(lines)
        self.wins = [(int(o), np.ascontiguousarray(d, F32).reshape(self.lines, -1)) for o, d in wins]
        end = 0
        for o, d in self.wins:
            assert end <= o and o + d.shape[1] <= self.n, (end, o, d.shape, self.n)
            end = o + d.shape[1]

    @classmethod
    def of_dense(cls, x, ranges):
        """the windows `ranges` = [(lo, hi)] of a dense [lines][n] array, which must be +0.0 outside them"""
        x = np.asarray(x, F32)
        x = x.reshape(-1, x.shape[-1])
        rest = x.view(np.uint32).copy()
        for lo, hi in ranges:
            rest[:, lo:hi] = 0
        assert not rest.any(), "the dense row is not +0.0 outside its windows"
        return cls(x.shape[1], [(lo, x[:, lo:hi]) for lo, hi in ranges if hi > lo], x.shape[0])

    def covered(self):
        """elements per line that lie in a window"""
        return sum(d.shape[1] for _, d in self.wins)

    def values(self):
        """every windowed value of every line, float32 [lines][covered]"""
        return np.concatenate([d for _, d in self.wins], axis=1) if self.wins else np.zeros((self.lines, 0), F32)

    def gather(self, idx):
        """float32 [lines] + idx.shape: the row at the positions idx (each in [0, n))"""
        idx = np.asarray(idx, np.int64)
        assert idx.size == 0 or (0 <= int(idx.min()) and int(idx.max()) < self.n), (int(idx.min()), int(idx.max()), self.n)
        out = np.zeros((self.lines,) + idx.shape, F32)
        for o, d in self.wins:
            m = (idx >= o) & (idx < o + d.shape[1])
            if m.any():
                out[:, m] = d[:, idx[m] - o]
        return out

    def take(self, lo, hi):
        """float32 [lines][hi - lo]: positions [lo, hi), 0 <= lo <= hi <= n"""
        assert 0 <= lo <= hi <= self.n, (lo, hi, self.n)
        return self.gather(np.arange(lo, hi, dtype=np.int64))

    def clipped(self, n):
        """the row cut to its first n elements"""
        assert 0 <= n <= self.n
        return SparseRow(n, [(o, d[:, :max(0, min(d.shape[1], n - o))]) for o, d in self.wins if o < n], self.lines)
