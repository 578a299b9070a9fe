"""Host reference of pcg_alert_cases (include/pcgnn.h): the slots of a member list grouped into the connected components of
"linked".  A union-find that always hangs the larger root under the smaller - so a component's root is its lowest slot - with a
"first slot of a node" dict.  Pure numpy / python: slow and plain on purpose."""
import numpy as np


def valid_slots(members, n_nodes):
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    return (members >= 0) & (members < n_nodes)


def group(csr, members, n_nodes, relations=None, labels=None):
    """csr: [(indptr, indices)] per relation; members: ids in alert order (-1 = padding, anything else outside [0, n_nodes) is
    treated as padding too); relations: None = all, else the selected relation numbers; labels: one per slot or None.
    -> dict(case_of [m], head [C], offsets [C + 1], order [m_valid], links [C], hits [C] or None, n_cases)."""
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    m = members.size
    rels = list(range(len(csr))) if relations is None else sorted({int(r) for r in relations})
    ok = valid_slots(members, n_nodes)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    first = {}
    for p in range(m):
        if ok[p]:
            first.setdefault(int(members[p]), p)
    slot_links = np.zeros(m, dtype=np.int64)
    for p in range(m):
        if not ok[p]:
            continue
        v = int(members[p])
        unite(p, first[v])
        for r in rels:
            indptr, indices = csr[r]
            for u in indices[indptr[v]:indptr[v + 1]].tolist():
                if u != v and u in first:
                    slot_links[p] += 1
                    unite(p, first[u])
    root = np.array([find(p) if ok[p] else -1 for p in range(m)], dtype=np.int64)
    head = np.array([p for p in range(m) if ok[p] and root[p] == p], dtype=np.int32)
    number = {int(h): c for c, h in enumerate(head)}
    case_of = np.array([number[int(root[p])] if ok[p] else -1 for p in range(m)], dtype=np.int32)
    C = head.size
    size = np.bincount(case_of[ok], minlength=C).astype(np.int64) if C else np.zeros(0, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
    slots = np.nonzero(ok)[0]
    order = slots[np.argsort(case_of[slots], kind="stable")].astype(np.int32)
    links = np.bincount(case_of[ok], weights=slot_links[ok], minlength=C).astype(np.int32) if C else np.zeros(0, dtype=np.int32)
    hits = None
    if labels is not None:
        lab = np.asarray(labels, dtype=np.int64).reshape(-1)
        hits = (np.bincount(case_of[ok], weights=(lab[ok] == 1), minlength=C).astype(np.int32) if C
                else np.zeros(0, dtype=np.int32))
    return dict(case_of=case_of, head=head, offsets=offsets, order=order, links=links, hits=hits, n_cases=int(C))


def brute_links(csr, members, n_nodes, relations, case_of, n_cases):
    """links by its definition, without the dict: per case, over its slots p and the selected relations, the CSR entries of
    members[p] whose target is a member node other than members[p]."""
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    ok = valid_slots(members, n_nodes)
    member_nodes = set(members[ok].tolist())
    rels = list(range(len(csr))) if relations is None else list(relations)
    out = np.zeros(n_cases, dtype=np.int32)
    for p in np.nonzero(ok)[0]:
        v = int(members[p])
        for r in rels:
            indptr, indices = csr[r]
            row = indices[indptr[v]:indptr[v + 1]]
            out[case_of[p]] += sum(1 for u in row.tolist() if u != v and u in member_nodes)
    return out


def scipy_partition(csr, members, n_nodes, relations=None):
    """The partition of the valid slots by scipy's connected_components on the induced, symmetrised slot graph (duplicate
    nodes joined) -> label per slot, -1 for padding."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    m = members.size
    ok = valid_slots(members, n_nodes)
    rels = list(range(len(csr))) if relations is None else list(relations)
    slots_of = {}
    for p in np.nonzero(ok)[0]:
        slots_of.setdefault(int(members[p]), []).append(int(p))
    rows, cols = [], []
    for v, ps in slots_of.items():
        for p in ps[1:]:
            rows.append(ps[0]), cols.append(p)
        for r in rels:
            indptr, indices = csr[r]
            for u in indices[indptr[v]:indptr[v + 1]].tolist():
                if u != v and u in slots_of:
                    rows.append(ps[0]), cols.append(slots_of[u][0])
    a = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, m)).tocsr()
    _, lab = connected_components(a + a.T, directed=False)
    return np.where(ok, lab, -1)


def same_partition(a, b) -> bool:
    """two labelings of the slots describe the same partition (-1 = in no part in both)"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    keep = a >= 0
    pairs = set(zip(a[keep].tolist(), b[keep].tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


def random_csr(rs, n, n_rel, avg_deg, symmetric=False, self_loops=True):
    """small random multi-relation CSR, rows sorted and de-duplicated; asymmetric unless asked"""
    out = []
    for _ in range(n_rel):
        e = int(n * avg_deg)
        src, dst = rs.randint(0, n, size=e), rs.randint(0, n, size=e)
        if symmetric:
            src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        if self_loops:
            src, dst = np.concatenate([src, np.arange(n)]), np.concatenate([dst, np.arange(n)])
        out.append(csr_from_pairs(n, src, dst))
    return out


def csr_from_pairs(n, src, dst):
    key = np.unique(np.asarray(src, dtype=np.int64) * n + np.asarray(dst, dtype=np.int64))
    rows, cols = key // n, (key % n).astype(np.int32)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr), cols
