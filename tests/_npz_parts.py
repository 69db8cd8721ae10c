"""Fixtures stored in parts, so that no file under tests/golden/ is larger than 1 MiB.

``save_npz_parts(path, **arrays)`` writes ``<stem>.npz`` and, when that would pass the limit,
``<stem>.part1.npz``, ``<stem>.part2.npz``, ...; an array too large for one part is flattened and cut
into ``<key>@@0``, ``<key>@@1``, ... beside its ``<key>@@shape``. ``load_npz_parts(path)`` puts them back
together: the same keys, dtypes and values that one ``np.load`` of an unsplit file would give."""
import io
import os
import re

import numpy as np

PART_LIMIT = 1000 * 1000  # bytes per file on disk, under 1 MiB with room to spare


class NpzParts(dict):
    """What np.load returns as far as the tests use it: item access, ``in``, ``.files``."""

    @property
    def files(self):
        return list(self.keys())


def _part_path(path, i):
    return path if i == 0 else path[:-len(".npz")] + f".part{i}.npz"


def _packed(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save_npz_parts(path, **arrays):
    assert path.endswith(".npz")
    pieces = []  # (key, array) in order, arrays above the limit cut into pieces
    for k, v in arrays.items():
        v = np.asarray(v)
        assert "@@" not in k
        n = -(-len(_packed({k: v})) // (PART_LIMIT // 2)) if v.ndim else 1
        if n <= 1:
            pieces.append((k, v))
        else:
            pieces.append((f"{k}@@shape", np.asarray(v.shape, dtype=np.int64)))
            pieces.extend((f"{k}@@{j}", c) for j, c in enumerate(np.array_split(v.reshape(-1), n)))
    parts, cur, size = [], {}, 0
    for k, v in pieces:  # a member's size alone bounds what it adds to an archive
        s = len(_packed({k: v}))
        if cur and size + s > PART_LIMIT:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += s
    parts.append(cur)
    i = len(parts)
    while os.path.exists(_part_path(path, i)):  # parts of an earlier, larger version
        os.remove(_part_path(path, i))
        i += 1
    for i, p in enumerate(parts):
        data = _packed(p)
        assert len(data) <= PART_LIMIT, (path, i, len(data))
        with open(_part_path(path, i), "wb") as f:
            f.write(data)
    return len(parts)


def load_npz_parts(path):
    out, cut = NpzParts(), {}
    i = 0
    while i == 0 or os.path.exists(_part_path(path, i)):
        with np.load(_part_path(path, i)) as z:
            for k in z.files:
                m = re.fullmatch(r"(.+)@@(\d+|shape)", k)
                if m:
                    cut.setdefault(m.group(1), {})[m.group(2)] = z[k]
                    out.setdefault(m.group(1), None)  # keeps the key's place in the order
                else:
                    out[k] = z[k]
        i += 1
    for k, rows in cut.items():
        out[k] = np.concatenate([rows[str(j)] for j in range(len(rows) - 1)]).reshape(tuple(rows["shape"]))
    return out
