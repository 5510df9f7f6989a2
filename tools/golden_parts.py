"""Golden fixtures stored in parts, so that no file under tests/golden/ exceeds
1 MiB: ``<name>.npz`` when the fixture fits, otherwise ``<name>.part00.npz``,
``<name>.part01.npz`` ... with the fixture's arrays distributed over them (each
array whole, in one part).  ``load`` gives the same mapping either way.

usage: python tools/golden_parts.py NAME ...   # re-pack tests/golden/NAME.npz in place, arrays unchanged
"""

import glob
import io
import os
import sys

import numpy as np

LIMIT = 1 << 20            # bytes a committed file may have
PACK = LIMIT - (64 << 10)  # fill parts up to here: room for the zip directory


class Parts:
    """Read-only mapping over the arrays of several .npz files (the NpzFile
    interface the tests use: ``z[key]``, ``key in z``, ``z.files``)."""

    def __init__(self, paths):
        self._z = [np.load(p) for p in paths]
        self._where = {k: z for z in self._z for k in z.files}
        self.files = [k for z in self._z for k in z.files]
        assert len(self.files) == len(self._where), "an array is stored in two parts"

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def keys(self):
        return list(self.files)


def part_paths(stem):
    return sorted(glob.glob(glob.escape(stem) + ".part[0-9][0-9].npz"))


def load(stem):
    """The fixture at ``stem`` (path without .npz), whole or in parts."""
    if os.path.exists(stem + ".npz"):
        return np.load(stem + ".npz")
    paths = part_paths(stem)
    if not paths:
        raise FileNotFoundError(stem + ".npz")
    return Parts(paths)


def _packed_size(key, value):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{key: value})
    return buf.getbuffer().nbytes


def save(stem, arrays):
    """Write the fixture: one compressed .npz when it stays within LIMIT,
    otherwise parts filled in the order of ``arrays``.  Replaces whatever form
    of the fixture was there.  Returns the paths written."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    bins, room = [[]], PACK
    for k, v in arrays.items():
        n = _packed_size(k, v)
        if n > PACK:
            raise ValueError(f"{k}: {n} bytes compressed, above the per-file limit")
        if n > room and bins[-1]:
            bins.append([])
            room = PACK
        bins[-1].append(k)
        room -= n
    for old in part_paths(stem) + [stem + ".npz"]:
        if os.path.exists(old):
            os.remove(old)
    names = [stem + ".npz"] if len(bins) == 1 else [f"{stem}.part{i:02d}.npz" for i in range(len(bins))]
    for path, keys in zip(names, bins):
        np.savez_compressed(path, **{k: arrays[k] for k in keys})
        assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    return names


def main():
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    for name in sys.argv[1:]:
        stem = os.path.join(golden, name)
        z = load(stem)
        arrays = {k: z[k] for k in z.files}
        for p in save(stem, arrays):
            print(p, os.path.getsize(p), "bytes")
        back = load(stem)
        assert sorted(back.files) == sorted(arrays)
        for k, v in arrays.items():
            w = back[k]
            assert w.dtype == v.dtype and w.shape == v.shape and w.tobytes() == v.tobytes(), k


if __name__ == "__main__":
    main()
