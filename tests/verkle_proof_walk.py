"""The tree-proof statement of include/vc_verkle.h restated over the oracle tree
(pyoracle.verkle.VerkleTree): the query list, the proof's commitment list and the depths of a set
of keys, and the key sets of the proof tests.

With `commit` the walk returns full queries (evaluations, commitment, z, y) for
pyoracle.protocol.prove_multiproof; without it only the counts (no commitment is needed to know how
many openings a proof holds). Test data only; never shipped.
"""
import random

from verkle32_keys import key_set, quirk_keys, value

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def keys_n3(seed, n_random=40):
    """random 3-byte keys, a third of them sharing the first byte (internal nodes below the root,
    level-skipping splits when the second byte is shared too), a few with last unit 0 (the only
    unit of c1 at N = 3)"""
    rng = random.Random(seed)
    keys = []
    for i in range(n_random):
        b = bytearray(rng.randrange(256) for _ in range(3))
        if i % 3 == 0:
            b[0] = 77
        if i % 9 == 0:
            b[1] = 5
        if i % 5 == 0:
            b[2] = 0
        keys.append(bytes(b))
    return keys


def tree_items(N, seed):
    """[(key, value)] of the proof tests' tree for key length N, the last one with an all-zero value"""
    rng = random.Random(seed)
    keys = key_set(seed, n_random=60) + quirk_keys()[0] if N == 32 else keys_n3(seed)
    items = [(k, value(rng)) for k in dict.fromkeys(keys)]
    zero_key = bytes([3] * N)
    return [kv for kv in items if kv[0] != zero_key] + [(zero_key, bytes(32))]


def build(N, seed, make_tree, skip_exc):
    """insert tree_items into make_tree(N), skipping the inserts that raise skip_exc (the
    reference's panics) -> (tree, [(key, value)] inserted)"""
    t, done = make_tree(N), []
    for k, v in tree_items(N, seed):
        try:
            t.insert_single(k, v)
        except skip_exc:
            continue
        done.append((k, v))
    return t, done


def provable(otree, items):
    """the inserted (key, value) pairs the oracle tree's get_single finds (a level-skipping split
    can hide a key, tests/verkle32_keys.py quirk_keys)"""
    return [(k, v) for k, v in items if otree.get_single(k) == v]


def _split(value32):
    return int.from_bytes(value32[:16], "little") % R, int.from_bytes(value32[16:32], "little") % R


def walk(otree, keys, commit=None):
    """-> {"depth", "n_com", "n_queries"} and, with commit, "queries" [(evals[256], C, z, y)] and
    "commitments" (the tree must be committed with the same commit)"""
    from pyoracle.arkser import to_data_item
    N = otree.N
    seen, com_seen, coms, queries, depth = set(), set(), [], [], []
    item_of = {}

    def item(node):
        if id(node) not in item_of:
            item_of[id(node)] = to_data_item(node.commit)
        return item_of[id(node)]

    def emit(ident, z, make):
        if (ident, z) in seen:
            return
        seen.add((ident, z))
        queries.append(make() if commit else None)

    def add_com(ident, make):
        if ident not in com_seen:
            com_seen.add(ident)
            coms.append(make() if commit else None)

    halves = {}

    def ext_rows(E):
        if id(E) not in halves:
            c1, c2 = [0] * N, [0] * N
            for index, leaf in E.leaves.items():
                lo, hi = _split(leaf)
                il, ih = (2 * index) % N, (2 * index + 1) % N
                if index < N // 2:
                    c1[il], c1[ih] = lo, hi
                else:
                    c2[il], c2[ih] = lo, hi
            halves[id(E)] = (c1, c2, commit(c1), commit(c2))
        return halves[id(E)]

    for K in keys:
        path, node = [], otree.root
        while not node.ext:
            path.append(node)
            node = node.children[K[len(path) - 1]]
        E, d = node, len(path)
        assert E.stem == tuple(K) and 1 <= d <= N - 1
        depth.append(d)
        u = K[-1]
        half = 1 if u < N // 2 else 2
        lo, hi = _split(otree.get_single(K))
        for j in range(1, d):
            add_com(id(path[j]), lambda j=j: path[j].commit)
        add_com(id(E), lambda: E.commit)
        add_com((id(E), half), lambda: ext_rows(E)[1 + half])
        nodes = path + [E]
        for j in range(d):
            def q1(j=j):
                ev = [0] * 256
                for k, ch in path[j].children.items():
                    ev[k] = item(ch)
                return (ev, path[j].commit, K[j], item(nodes[j + 1]))
            emit(id(path[j]), K[j], q1)
        stem_item = int.from_bytes(bytes(K), "little") % R

        def qe(z, y):
            c1, c2, C1, C2 = ext_rows(E)
            ev = [1, stem_item, to_data_item(C1), to_data_item(C2)] + [0] * 252
            return (ev, E.commit, z, y() if callable(y) else y)
        emit(id(E), 0, lambda: qe(0, 1))
        emit(id(E), 1, lambda: qe(1, stem_item))
        emit(id(E), 1 + half, lambda: qe(1 + half, lambda: to_data_item(ext_rows(E)[1 + half])))

        def qh(z, y):
            rows = ext_rows(E)
            return (rows[half - 1] + [0] * (256 - N), rows[1 + half], z, y)
        emit((id(E), half), (2 * u) % N, lambda: qh((2 * u) % N, lo))
        emit((id(E), half), (2 * u + 1) % N, lambda: qh((2 * u + 1) % N, hi))
    out = {"depth": depth, "n_com": len(coms), "n_queries": len(queries)}
    if commit:
        out["queries"], out["commitments"] = queries, coms
    return out
