"""The plain statement of the hash join that tests/test_gpu_join_edges.py holds the device to. No device code, no oracle.

Keys are rows of KW u64 words (a numpy array of shape (n, KW), KW in {1, 2, 4}) or a list of `bytes` (the join on serialized keys).
A validity is a bool array or None (= every row valid). A row with validity 0 never matches, on either side. Pairs are
(probe_idx, build_row) as two u32 arrays sorted by (probe_idx, build_row) — the order dbhip_join_probe promises.

inner_pairs_dict is the definition: a dictionary from the key to the build rows that carry it. inner_pairs_fast is its vectorised twin
for the cases with millions of rows (a stable sort of the build keys, two binary searches per probe row); tests/test_join_ref_cpu.py
shows that the two agree on every case both can take and that both agree with the C oracle's orc_join_inner_u64 on one-word keys."""
import numpy as np

KINDS = ("inner", "left", "left_semi", "left_anti", "right", "right_semi", "right_anti", "full")
DICT_MAX_ROWS = 200_000     # inner_pairs takes the dictionary form up to this many rows (both sides together)


def _is_bytes(keys):
    return isinstance(keys, (list, tuple))


def _rows2d(keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return k.reshape(len(k), k.shape[1] if k.ndim > 1 else 1)


def key_rows(keys):
    """the keys as hashable Python values: bytes as they are, u64 rows as tuples of ints"""
    if _is_bytes(keys):
        return list(keys)
    k = _rows2d(keys)
    return [tuple(r) for r in k.tolist()]


def _valid(valid, n):
    return np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)


def _pairs(p, b):
    return np.asarray(p, dtype=np.uint32), np.asarray(b, dtype=np.uint32)


def inner_pairs_dict(build_keys, build_valid, probe_keys, probe_valid, key=None):
    """The definition. `key` (tests of the case tables only) maps a key row to what is compared instead of the whole row."""
    brows, prows = key_rows(build_keys), key_rows(probe_keys)
    bv, pv = _valid(build_valid, len(brows)), _valid(probe_valid, len(prows))
    key = key or (lambda r: r)
    table = {}
    for b, r in enumerate(brows):
        if bv[b]:
            table.setdefault(key(r), []).append(b)
    op, ob = [], []
    for p, r in enumerate(prows):
        if pv[p]:
            rows = table.get(key(r))
            if rows:
                op += [p] * len(rows)
                ob += rows
    return _pairs(op, ob)


def key_ids(build_keys, probe_keys):
    """one u64 id per key row, equal ids <=> equal rows (the two sides are numbered together)"""
    if _is_bytes(build_keys):
        ids = {}
        both = [ids.setdefault(r, len(ids)) for r in list(build_keys) + list(probe_keys)]
        both = np.array(both, dtype=np.uint64)
        return both[:len(build_keys)], both[len(build_keys):]
    bk, pk = _rows2d(build_keys), _rows2d(probe_keys)
    kw = max(bk.shape[1], pk.shape[1])
    if kw == 1:
        return bk.reshape(-1), pk.reshape(-1)
    both = np.ascontiguousarray(np.concatenate([bk.reshape(-1, kw), pk.reshape(-1, kw)]))
    _, inv = np.unique(both.view(np.dtype((np.void, 8 * kw))).reshape(-1), return_inverse=True)
    inv = inv.reshape(-1).astype(np.uint64)
    return inv[:len(bk)], inv[len(bk):]


def inner_pairs_fast(build_keys, build_valid, probe_keys, probe_valid):
    """The vectorised twin: the valid build rows stably sorted by key id (rows of one key stay ascending), the run of every probe
    key found by two binary searches, the runs written out probe row after probe row."""
    bid, pid = key_ids(build_keys, probe_keys)
    bv, pv = _valid(build_valid, len(bid)), _valid(probe_valid, len(pid))
    rows = np.flatnonzero(bv)
    order = rows[np.argsort(bid[rows], kind="stable")]
    sorted_ids = bid[order]
    lo = np.searchsorted(sorted_ids, pid, side="left")
    cnt = np.searchsorted(sorted_ids, pid, side="right") - lo
    cnt[~pv] = 0
    hit = np.flatnonzero(cnt)
    c = cnt[hit]
    total = int(c.sum())
    start = np.cumsum(c) - c
    within = np.arange(total, dtype=np.int64) - np.repeat(start, c)
    return _pairs(np.repeat(hit, c), order[np.repeat(lo[hit], c) + within] if total else [])


def inner_pairs(build_keys, build_valid, probe_keys, probe_valid):
    small = len(build_keys) + len(probe_keys) <= DICT_MAX_ROWS
    return (inner_pairs_dict if small else inner_pairs_fast)(build_keys, build_valid, probe_keys, probe_valid)


def matched_probe(build_keys, build_valid, probe_keys, probe_valid):
    """bool[n]: the probe row has at least one build partner (dbhip_join_probe_mark)"""
    p, _ = inner_pairs(build_keys, build_valid, probe_keys, probe_valid)
    out = np.zeros(len(probe_keys), dtype=bool)
    out[p] = True
    return out


def matched_build(pairs, nb):
    """bool[nb]: the build row is in some pair (dbhip_join_mark_build / dbhip_join_build_matched)"""
    out = np.zeros(nb, dtype=bool)
    out[np.asarray(pairs[1], dtype=np.int64)] = True
    return out


def join_rows(kind, build_keys, build_valid, probe_keys, probe_valid):
    """The output rows of one probe block followed by the rows of final_probe, as (probe_idx, build_row) i64 arrays with -1 for the
    NULL side (and for the side a semi / anti join does not return). Order: the pairs by (probe_idx, build_row), then the unmatched
    probe rows ascending (left, full), then the build rows of final_probe ascending (right kinds, full)."""
    assert kind in KINDS, kind
    n, nb = len(probe_keys), len(build_keys)
    p, b = inner_pairs(build_keys, build_valid, probe_keys, probe_valid)
    p, b = p.astype(np.int64), b.astype(np.int64)
    mp = np.zeros(n, dtype=bool)
    mp[p] = True
    mb = matched_build((p, b), nb)
    none = lambda k: np.full(k, -1, dtype=np.int64)   # noqa: E731
    if kind == "left_semi":
        rows = np.flatnonzero(mp)
        return rows, none(len(rows))
    if kind == "left_anti":
        rows = np.flatnonzero(~mp)
        return rows, none(len(rows))
    if kind == "right_semi":
        rows = np.flatnonzero(mb)
        return none(len(rows)), rows
    if kind == "right_anti":
        rows = np.flatnonzero(~mb)
        return none(len(rows)), rows
    op, ob = [p], [b]
    if kind in ("left", "full"):
        rows = np.flatnonzero(~mp)
        op.append(rows)
        ob.append(none(len(rows)))
    if kind in ("right", "full"):
        rows = np.flatnonzero(~mb)
        op.append(none(len(rows)))
        ob.append(rows)
    return np.concatenate(op), np.concatenate(ob)


def bits_set(indices, nbits):
    """bool[nbits]: bit i is set iff i is among the indices; indices >= nbits are ignored (dbhip_bitmap_set_indices)"""
    out = np.zeros(nbits, dtype=bool)
    idx = np.asarray(indices, dtype=np.int64)
    out[idx[idx < nbits]] = True
    return out
