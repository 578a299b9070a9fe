"""Host reference of the halo exchange of the node-partitioned path, written from the contract in include/pcgnn.h
("multi-GPU halo exchange helpers") - numpy only, integers and float64.  The order of the ids inside an owner's range of
the request list is whatever the device's atomics gave, so everything here compares SETS, never positions."""
import numpy as np

MISS = -1
HALO_MAX_PROBE = 128


def remote_set(csr_rows, centres, lo, hi, n_local, pos_ids):
    """The sorted distinct neighbours - over all relations of csr_rows = [(indptr, indices)] (local rows, global ids) - of the
    `centres` (local row numbers; outside [0, n_local): nothing; duplicates: once) that this rank does not own ([lo, hi)) and
    that are not train positives."""
    c = np.unique(np.asarray(centres, dtype=np.int64).reshape(-1))
    c = c[(c >= 0) & (c < n_local)]
    got = [np.zeros(0, np.int64)]
    for indptr, indices in csr_rows:
        for v in c.tolist():
            got.append(np.asarray(indices[int(indptr[v]):int(indptr[v + 1])], dtype=np.int64))
    ids = np.unique(np.concatenate(got))
    ids = ids[(ids < lo) | (ids >= hi)]
    return np.setdiff1d(ids, np.asarray(pos_ids, dtype=np.int64).reshape(-1))


def owner(bounds, id):
    """The largest r with bounds[r] <= id (r < world): an empty shard [b, b) never owns b - the next non-empty one does."""
    bounds = [int(b) for b in bounds]
    r = 0
    for k in range(len(bounds) - 1):
        if bounds[k] <= id:
            r = k
    return r


def owners(bounds, ids):
    return np.array([owner(bounds, int(i)) for i in np.asarray(ids).reshape(-1)], dtype=np.int64)


def halo_hash(x):
    """halo_map.h's hash, in numpy - ONLY to choose inputs whose home slots collide; no expected value comes from it."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def owner_ranges(world, self_rank, pitch, per_owner):
    """[begin, end) of every owner's range of the request list (self: an empty range in the pitched layout)"""
    out, run = [], 0
    for o in range(world):
        if pitch > 0:
            j = o - (1 if o > self_rank else 0)
            out.append((j * pitch, (j + 1) * pitch) if (o != self_rank or world == 1) else (0, 0))
        else:
            out.append((run, run + int(per_owner[o])))
            run += int(per_owner[o])
    return out


def check_collect(uniq, counts, keys, vals, expected, bounds, pitch, halo_cap, world, self_rank):
    """Assert everything the contract says about the state a pcg_halo_collect leaves: uniq [halo_cap] int32, counts [131],
    the two halves of the hash table (uint32 views), against the expected id set.  Returns {id: slot} of the ids with a slot."""
    uniq = np.asarray(uniq, dtype=np.int64)
    keys = np.asarray(keys).astype(np.int64) & 0xFFFFFFFF
    vals = np.asarray(vals).astype(np.int64) & 0xFFFFFFFF
    expected = np.unique(np.asarray(expected, dtype=np.int64))           # (a set: sorted, once each)
    assert uniq.shape[0] == halo_cap
    own = owners(bounds, expected)
    per_owner = np.bincount(own, minlength=world)[:world]
    assert per_owner[self_rank] == 0, "the reference itself: nothing owned is remote"
    assert np.array_equal(np.asarray(counts[:world], dtype=np.int64), per_owner), \
        f"counts[0:world] {np.asarray(counts[:world]).tolist()} != per-owner sizes {per_owner.tolist()}"
    ranges = owner_ranges(world, self_rank, pitch, per_owner)
    packed_over = pitch == 0 and expected.size > halo_cap
    used = np.zeros(halo_cap, dtype=bool)
    slot_of = {}
    for o in range(world):
        want = set(expected[own == o].tolist())
        if packed_over:
            continue
        b, e = ranges[o]
        assert 0 <= b <= e <= halo_cap, (o, b, e)
        seg = uniq[b:e]
        got = seg[seg >= 0]
        assert len(set(got.tolist())) == got.size, f"owner {o}: an id sits in two slots"
        used[b:e] |= seg >= 0
        if pitch > 0 and len(want) > pitch:
            assert got.size == pitch and set(got.tolist()) <= want, \
                f"owner {o} over its pitch: exactly {pitch} of its ids get slots ({got.size} did)"
        else:
            assert set(got.tolist()) == want, f"owner {o}: request range holds {sorted(set(got.tolist()) ^ want)[:8]} wrongly"
        for i in np.flatnonzero(seg >= 0).tolist():
            slot_of[int(seg[i])] = b + i
    if packed_over:
        assert np.all(uniq == -1), "packed layout over halo_cap: no id gets a slot"
    assert np.all(uniq[~used] == -1), "every request entry outside the owners' filled slots is -1"
    assert int((uniq >= 0).sum()) == len(slot_of)
    # the table: its keys are exactly the expected ids, once each; an id with a slot is found with vals == slot
    occ = keys != 0xFFFFFFFF
    assert np.array_equal(np.sort(keys[occ]), expected), "the table's keys are the expected ids, once each, and nothing else"
    at = {int(k): int(h) for h, k in zip(np.flatnonzero(occ).tolist(), keys[occ].tolist())}
    for i in expected.tolist():
        v = int(vals[at[i]])
        if i in slot_of:
            assert v == slot_of[i] and int(uniq[v]) == i, f"id {i}: vals {v}, slot {slot_of[i]}"
        else:
            assert v >= halo_cap, f"id {i} has no request slot, yet the table names slot {v}"
    return slot_of


def translate(id, lo, hi, n_local, pos_ids, pos_idx, slot_of, halo_base=None):
    """Row of [owned | train-pos | halo] of a list entry, or MISS: owned first, then a fetched slot, then train-pos
    (halo_translate's order).  slot_of: {id: halo slot}; halo_base defaults to n_local + len(pos_ids).  A negative entry (a
    hole) stays as it is."""
    id = int(id)
    if id < 0:
        return id
    if halo_base is None:
        halo_base = n_local + len(pos_ids)
    if lo <= id < hi:
        return id - lo
    if id in slot_of:
        return halo_base + int(slot_of[id])
    pos_ids = np.asarray(pos_ids, dtype=np.int64).reshape(-1)
    at = int(np.searchsorted(pos_ids, id))
    if at < pos_ids.size and int(pos_ids[at]) == id:
        return n_local + int(np.asarray(pos_idx).reshape(-1)[at])
    return MISS


def mean_f64(rows, cnt):
    """float64 sum over the feature rows that were found (a missed id is left out by the caller) / the device's cnt - the
    divisor stays the row's count"""
    rows = np.asarray(rows, dtype=np.float64)
    s = rows.sum(axis=0) if rows.size else np.zeros(rows.shape[-1] if rows.ndim == 2 else 0, np.float64)
    return s / float(cnt)


def mean_bound(rows, cnt):
    """Per element: the worst-case error of an f32 sum of `rows` in any order plus the division's rounding,
    (cnt + 1) * 2^-24 * sum_j |x_jf| / cnt, in float64."""
    rows = np.abs(np.asarray(rows, dtype=np.float64))
    return (cnt + 1) * 2.0 ** -24 * rows.sum(axis=0) / float(cnt)
