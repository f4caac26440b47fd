"""A plain Python model of the filter's feature table (csrc/ekf_feature_table.hpp) and the writer of the operation
sequences tools/filter_host_check.cpp replays: after every operation the expected columns, and after a compaction the
expected msrc / mconv.  The GPU test of the records (tests/test_gpu_end_update.py) uses the same model.
Usage: python tools/filter_host_check.py OUT_DIR"""
import os, struct, sys


class FeatureModel:
    """One list per column; `n` is the state dimension, `next_real` the next real_index."""
    COLUMNS = ("pos", "coding", "real_index", "n_find", "n_tot", "center", "inn", "rem")

    def __init__(self, camera_dim=13):
        self.camera_dim, self.n, self.next_real = camera_dim, camera_dim, 1
        for c in self.COLUMNS:
            setattr(self, c, [])

    def __len__(self):
        return len(self.pos)

    def add(self, u, v):
        for c, x in zip(self.COLUMNS, (self.n, 0, self.next_real, 1, 1, (u, v), 0, 0)):
            getattr(self, c).append(x)
        self.next_real += 1
        self.n += 6

    def compact(self, remove=(), convert=()):
        """Drops `remove`, makes `convert` XYZ features; returns (msrc, mconv) of the state rows."""
        msrc, mconv = list(range(self.camera_dim)), [-1] * self.camera_dim
        keep = [i for i in range(len(self)) if i not in remove]
        pos, coding = [], []
        for i in keep:
            pos.append(len(msrc))
            if i in convert:
                msrc += [self.pos[i]] * 3
                mconv += [3 * i, 3 * i + 1, 3 * i + 2]
            else:
                fs = 3 if self.coding[i] else 6
                msrc += [self.pos[i] + e for e in range(fs)]
                mconv += [-1] * fs
            coding.append(1 if i in convert else self.coding[i])
        for c in self.COLUMNS[2:]:
            setattr(self, c, [getattr(self, c)[i] for i in keep])
        self.pos, self.coding, self.n = pos, coding, len(msrc)
        return msrc, mconv

    def fold(self, bits):
        """Device track bits: bit 0 is the visibility, bit 1 sets the sticky removal flag."""
        self.inn = [b & 1 for b in bits]
        self.rem = [r | ((b >> 1) & 1) for r, b in zip(self.rem, bits)]

    def set_meta(self, i, real_index=-1, n_find=-1):
        if real_index >= 0: self.real_index[i] = real_index
        if n_find >= 0: self.n_find[i] = n_find

    def set_track(self, i, n_tot=-1, in_innovation=-1, center=None, remove_flag=-1):
        if n_tot >= 0: self.n_tot[i] = n_tot
        if in_innovation >= 0: self.inn[i] = 1 if in_innovation else 0
        if center is not None: self.center[i] = tuple(center)
        if remove_flag >= 0: self.rem[i] = 1 if remove_flag else 0

    def searched(self, i, found, u, v):
        """Patch::findMatch of a searched feature: counted, centred on the match or (-1, -1); a miss leaves the innovation."""
        self.n_tot[i] += 1
        self.center[i] = (u, v) if found else (-1.0, -1.0)
        if not found: self.inn[i] = 0

    def count_found(self, i):
        self.n_find[i] += 1

    def flag_removal(self, i):
        self.rem[i] = 1


OP_ADD, OP_COMPACT, OP_FOLD, OP_META, OP_TRACK, OP_SEARCHED, OP_FOUND, OP_FLAG = 1, 2, 3, 4, 5, 6, 7, 8


class Recorder:
    """Applies operations to a model and writes them with the expected table behind each: int32 words, floats by their bits."""
    def __init__(self, camera_dim):
        self.m, self.words, self.ops = FeatureModel(camera_dim), [], 0

    def _f(self, x):
        return struct.unpack("<i", struct.pack("<f", x))[0]

    def _state(self, maps=None):
        m = self.m
        cen = [self._f(x) for uv in m.center for x in uv]
        self.words += [len(m), m.next_real] + m.pos + m.coding + m.real_index + m.n_find + m.n_tot + cen + m.inn + m.rem
        if maps is not None:
            self.words += [len(maps[0])] + maps[0] + maps[1]
        self.ops += 1

    def add(self, u, v):
        self.words += [OP_ADD, self.m.n, self._f(u), self._f(v)]
        self.m.add(u, v)
        self._state()

    def compact(self, remove=(), convert=()):
        N = len(self.m)
        self.words += [OP_COMPACT] + [int(i in remove) for i in range(N)] + [int(i in convert) for i in range(N)]
        self._state(self.m.compact(remove, convert))

    def fold(self, bits):
        self.words += [OP_FOLD] + list(bits)
        self.m.fold(bits)
        self._state()

    def set_meta(self, i, real_index=-1, n_find=-1):
        self.words += [OP_META, i, real_index, n_find]
        self.m.set_meta(i, real_index, n_find)
        self._state()

    def set_track(self, i, n_tot=-1, in_innovation=-1, center=None, remove_flag=-1):
        c = center if center is not None else (0.0, 0.0)
        self.words += [OP_TRACK, i, n_tot, in_innovation, int(center is not None), self._f(c[0]), self._f(c[1]), remove_flag]
        self.m.set_track(i, n_tot, in_innovation, center, remove_flag)
        self._state()

    def searched(self, i, found, u, v):
        self.words += [OP_SEARCHED, i, int(found), self._f(u), self._f(v)]
        self.m.searched(i, found, u, v)
        self._state()

    def count_found(self, i):
        self.words += [OP_FOUND, i]
        self.m.count_found(i)
        self._state()

    def flag_removal(self, i):
        self.words += [OP_FLAG, i]
        self.m.flag_removal(i)
        self._state()

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(struct.pack("<%di" % (2 + len(self.words)), self.m.camera_dim, self.ops, *self.words))


def _adds(r, count, first=0):
    for k in range(first, first + count):
        r.add(40.5 + 7 * k, 30.25 + 3 * k)


def _distinct(r):
    for i in range(len(r.m)):
        r.set_meta(i, real_index=100 + 3 * i, n_find=2 + i)
        r.set_track(i, n_tot=9 + i, in_innovation=i % 2, center=(1.5 * i, -2.0 - i), remove_flag=int(i % 3 == 0))


def seq_empty(r):                       # nothing to compact, nothing to fold
    r.compact()
    r.fold([])
    r.add(12.0, 13.0)
    r.compact()


def seq_remove_all(r):                  # the table goes back to empty; real indices go on counting
    _adds(r, 5)
    _distinct(r)
    r.compact(remove=range(5))
    r.compact()
    _adds(r, 2, 5)
    r.compact(remove=[0, 1])


def seq_remove_first_and_last(r):       # both ends of the columns
    _adds(r, 6)
    _distinct(r)
    r.compact(remove=[0, 5])
    r.compact(remove=[0, 3])
    r.compact(remove=[0])
    r.compact(remove=[0])


def seq_convert_then_remove(r):         # 3-state and 6-state features mixed
    _adds(r, 6)
    _distinct(r)
    r.compact(convert=[1, 3])
    _adds(r, 1, 6)
    r.compact(remove=[1, 2])            # a converted feature and an inverse-depth one
    r.compact(remove=[3], convert=[0, 4])   # removal and conversion in one pass; the last feature converted
    r.compact(convert=[2])              # the last inverse-depth feature: every feature has 3 states now
    r.compact(remove=[0, 1, 2, 3])


def seq_sticky_fold(r):                 # bit 1 on a feature that is flagged already; bit 1 clear never clears the flag
    _adds(r, 4)
    r.fold([2, 0, 3, 1])
    r.fold([2, 1, 0, 2])
    r.fold([0, 0, 0, 0])
    r.set_track(0, remove_flag=0)       # only the setter clears it
    r.fold([1, 1, 1, 1])
    r.fold([3, 0, 0, 0])
    r.compact(remove=[1])
    r.fold([0, 2, 1])


def seq_match_and_quality(r):           # what a frame does to the records: search results, found counts, the quality flag
    _adds(r, 4)
    r.fold([1, 1, 0, 1])
    r.searched(0, True, 101.5, 77.25)
    r.searched(1, False, 5.0, 6.0)      # a miss: centre (-1, -1), out of the innovation
    r.searched(3, True, 0.0, 239.0)
    r.count_found(0)
    r.count_found(3)
    r.count_found(3)
    r.flag_removal(1)
    r.flag_removal(1)                   # (twice is once)
    r.compact(remove=[1])
    r.searched(2, False, 1.0, 1.0)      # the last feature, after the compaction
    r.count_found(0)


SEQUENCES = {"match_and_quality": (seq_match_and_quality, 14), "empty_cam13": (seq_empty, 13), "empty_cam14": (seq_empty, 14), "remove_all": (seq_remove_all, 14),
             "remove_first_and_last": (seq_remove_first_and_last, 14), "convert_then_remove_cam13": (seq_convert_then_remove, 13),
             "convert_then_remove_cam14": (seq_convert_then_remove, 14), "sticky_fold": (seq_sticky_fold, 13)}


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, (seq, camera_dim) in SEQUENCES.items():
        r = Recorder(camera_dim)
        seq(r)
        r.write(os.path.join(out, name + ".bin"))
        print(name, r.ops, "operations")


if __name__ == "__main__":
    main(sys.argv[1])
