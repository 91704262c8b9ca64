"""The verkle commitment's host integer logic without a GPU (csrc/verkle_trie.hpp, verkle_rows.hpp,
verkle_plan.hpp): tests/cpp/verkle_plan_check.cpp, built with g++ and the address / undefined-
behaviour sanitizers and run directly, gets the keys this test inserts into the oracle tree
(oracle/pyoracle/verkle.py) in rounds and prints, per round, the device path's extension stage, the
delta plan and every internal level's lists, nodes named by their walk path from the root. Checked
here: the c1 / c2 rows against the oracle's placement of the leaves (node.rs:226-239), the stage's
layout, one part against several; the levels' order, rows and children against the oracle's nodes;
which rows are delta rows, their columns, snapshot indices and add ids; the plan's scratch reset;
a failed commitment (drop_delta) making the touched nodes' next rows full."""
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("verkle_plan") / "verkle_plan_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "verkle_plan_check.cpp"), "-o", str(exe)])
    return str(exe)


def _value(rng, i):
    """random values, some with a zero half or all zero (zero scalars are left out of the rows)"""
    v = bytearray(rng.randrange(256) for _ in range(32))
    if i % 5 == 1:
        v[:16] = bytes(16)
    elif i % 5 == 3:
        v[16:] = bytes(16)
    elif i % 11 == 4:
        v = bytearray(32)
    return bytes(v)


def _nodes(o):
    """path -> node of the oracle tree, and id(node) -> path"""
    by_path, path_of, stack = {}, {}, [((), o.root)]
    while stack:
        p, n = stack.pop()
        by_path[p] = n
        path_of[id(n)] = p
        if not n.ext:
            stack.extend((p + (u,), c) for u, c in n.children.items())
    return by_path, path_of


def _accepted(o, draws, rng, salt):
    """the draws the oracle accepts (the reference panics on the others), inserted into it"""
    from pyoracle import verkle as ov
    out = []
    for i, k in enumerate(draws):
        v = _value(rng, i + salt)
        try:
            o.insert_single(tuple(k), v)
        except ov.VerklePanic:
            continue
        out.append((bytes(k), v))
    return out


def _check_ext(N, stage, dirty_ext):
    E, nnz, rp = stage["E"], stage["nnz"], stage["row_ptr"]
    assert E == len(dirty_ext) == len(stage["ids"]) == len(stage["stems"])
    assert sorted(map(tuple, stage["ids"])) == sorted(dirty_ext)        # every dirty extension once
    assert len(rp) == 2 * E + 1 and rp[0] == 0 and rp[-1] == nnz == len(stage["cols"]) == len(stage["vals"])
    assert all(a <= b for a, b in zip(rp, rp[1:]))
    assert stage["maxlen"] == max(b - a for a, b in zip(rp, rp[1:]))
    assert stage["o_stem"] == (2 * E + 1) * 8 and stage["o_vals"] == stage["o_stem"] + 32 * E
    assert stage["o_ids"] == stage["o_vals"] + 16 * nnz and stage["o_cols"] == stage["o_ids"] + 4 * E
    assert stage["o_end"] == stage["o_cols"] + 4 * nnz == stage["size"]
    for e, p in enumerate(stage["ids"]):
        node = dirty_ext[tuple(p)]
        assert stage["stems"][e] == (bytes(node.stem) + bytes(32 - N)).hex()
        halves = ({}, {})   # position -> 16 bytes, in first-write order; a later write overwrites
        for index, leaf in node.leaves.items():
            h = halves[0 if index < N // 2 else 1]
            h[(2 * index) % N] = leaf[:16]
            h[(2 * index + 1) % N] = leaf[16:32]
        for r in range(2):
            want = [(c, v.hex()) for c, v in halves[r].items() if any(v)]
            a, b = rp[2 * e + r], rp[2 * e + r + 1]
            assert list(zip(stage["cols"][a:b], stage["vals"][a:b])) == want, (p, r)


def _check_round(N, dense_mode, out, o, inserted, before, base):
    """out: the check's JSON of this round; inserted: this round's keys in order; before: path ->
    {unit: child node} of the internal nodes at the round's start; base: the paths whose stored
    commitment is a delta base"""
    by_path, path_of = _nodes(o)
    dirty_ext = {p: n for p, n in by_path.items() if n.ext and not n.has_commit}
    dirty_int = {p: n for p, n in by_path.items() if not n.ext and not n.has_commit}
    a, b = out["ext"]
    assert a["workers"] == 4 and b["workers"] == 1 and b["parts"] == 1
    assert {k: v for k, v in a.items() if k not in ("workers", "parts")} == \
           {k: v for k, v in b.items() if k not in ("workers", "parts")}
    _check_ext(N, a, dirty_ext)
    levels = out["levels"]
    assert [L["level"] for L in levels] == sorted({len(p) for p in dirty_int}, reverse=True)  # deepest first
    assert sorted(tuple(p) for L in levels for p in L["ids"]) == sorted(dirty_int)           # each once
    assert len(set(out["snap_ids"])) == len(out["snap_ids"])
    assert out["scratch_live"] == out["plans"] + len(out["snap_ids"]) and out["scratch_after"] == 0
    n_delta = 0
    for L in levels:
        B, nnz, ptr, nz1 = L["B"], L["nnz"], L["ptr"], max(L["nnz"], 1)
        assert B == len(L["ids"]) and len(ptr) == B + 1 and ptr[0] == 0 and ptr[-1] == nnz == len(L["cols"])
        assert L["dense"] == (dense_mode == 1 or (dense_mode != 0 and B <= 64))
        assert L["o_child"] == 4 * nz1 and L["o_ids"] == 8 * nz1 and L["o_sidx"] == L["o_ids"] + 4 * B
        extra = (4 * nz1, 4 * B) if L["any_delta"] else (0, 0)
        assert L["o_add"] == L["o_sidx"] + extra[0] and L["o_end"] == L["o_add"] + extra[1] == L["size"]
        any_delta = False
        for r, p in enumerate(map(tuple, L["ids"])):
            assert len(p) == L["level"]
            cols, child = L["cols"][ptr[r]:ptr[r + 1]], L["child"][ptr[r]:ptr[r + 1]]
            assert [tuple(c) for c in child] == [p + (c,) for c in cols]   # the unit's subtree
            passing = [k[len(p)] for k in inserted if tuple(k[:len(p)]) == p]
            if p in base and not L["dense"] and passing:   # a delta row: the changed slots, first-insert order
                any_delta = True
                n_delta += 1
                assert L["any_delta"] and cols == list(dict.fromkeys(passing)), p
                assert L["add"][r] == list(p)
                for c, s in zip(cols, L["sidx"][ptr[r]:ptr[r + 1]]):
                    old = before[p].get(c)
                    if old is None:
                        assert s == -1, (p, c)
                    else:   # the child that held the slot at the last commitment, wherever it is now
                        assert s >= 0 and tuple(out["snap"][s]) == path_of[id(old)], (p, c)
            else:           # a full row: the node's children, sorted by unit
                assert cols == sorted(by_path[p].children), p
                if L["any_delta"]:
                    assert L["add"][r] is None and set(L["sidx"][ptr[r]:ptr[r + 1]]) <= {-1}
        assert L["any_delta"] == any_delta
    return n_delta


def _run(check_exe, N, dense_mode, rounds, afters=None):
    """rounds: lists of key draws. Returns the delta rows seen per round."""
    from pyoracle import verkle as ov
    afters = afters or [1] * len(rounds)
    o, rng = ov.VerkleTree(N), random.Random(N)
    fed, text = [], []
    for r, draws in enumerate(rounds):   # the oracle is rebuilt below: here only which keys are accepted
        kv = _accepted(o, draws, rng, 100 * r)
        fed.append(kv)
        text.append(f"{len(kv)} {afters[r]}\n" + "".join(f"{k.hex()} {v.hex()}\n" for k, v in kv))
    res = subprocess.run([check_exe], input=f"{N} {dense_mode} {len(rounds)}\n" + "".join(text), text=True,
                         capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    outs = [json.loads(line) for line in res.stdout.splitlines()]
    assert len(outs) == len(rounds)
    o, base, pending, deltas = ov.VerkleTree(N), set(), [], []
    for r, kv in enumerate(fed):
        by_path, _ = _nodes(o)
        before = {p: dict(n.children) for p, n in by_path.items() if not n.ext}
        for k, v in kv:
            o.insert_single(tuple(k), v)
        # (a failed commitment clears the slot log: only this round's inserts are planned, and the nodes
        # dirty at the failure are no bases any more)
        deltas.append(_check_round(N, dense_mode, outs[r], o, [k for k, _ in kv], before, base))
        by_path, _ = _nodes(o)
        dirty = {p for p, n in by_path.items() if not n.has_commit}
        if afters[r]:
            for n in by_path.values():
                n.has_commit = True
            base = {p for p, n in by_path.items() if not n.ext}
        else:
            base -= dirty
    return deltas, outs


def _draws(rng, N, arity, n):
    return [bytes(rng.randrange(arity) for _ in range(N)) for _ in range(n)]


@pytest.mark.parametrize("N,arity,n,upd", [(3, 6, 60, 6), (4, 4, 50, 5)])
def test_small_trees_delta_rows(check_exe, N, arity, n, upd):
    """heavy prefix sharing, dense forced off so that delta rows exist at these sizes: a first round
    and two update rounds"""
    rng = random.Random(N * 10 + arity)
    rounds = [_draws(rng, N, arity, n), _draws(rng, N, arity, upd), _draws(rng, N, arity, upd)]
    deltas, _ = _run(check_exe, N, 0, rounds)
    assert deltas[0] == 0 and deltas[1] > 0 and deltas[2] > 0


@pytest.mark.parametrize("N,arity,n,upd", [(3, 6, 60, 6), (4, 4, 50, 5)])
def test_failed_commit_recommits_in_full(check_exe, N, arity, n, upd):
    """drop_delta() in place of clear_dirty() after the first update round: every node that round
    touched (the root among them) gets a full row in the next, where a delta row stood otherwise"""
    rng = random.Random(N * 10 + arity)
    rounds = [_draws(rng, N, arity, n), _draws(rng, N, arity, upd), _draws(rng, N, arity, upd)]
    ok, _ = _run(check_exe, N, 0, rounds)
    failed, outs = _run(check_exe, N, 0, rounds, afters=[1, 0, 1])
    assert failed[1] == ok[1] > 0 and failed[2] < ok[2]
    touched = {tuple(p) for L in outs[1]["levels"] for p in L["ids"]}
    for L in outs[2]["levels"]:
        for r, p in enumerate(L["ids"]):
            if tuple(p) in touched and L["any_delta"]:
                assert L["add"][r] is None
    assert () in touched


def test_key32_sets_and_the_quirk_update(check_exe):
    """the key-length-32 parity tests' stems (every branch of the stem reduction, c1 and c2 slots) and
    the level-skipping quirk's re-insert as the update round; levels of <= 64 rows stay dense"""
    from verkle32_keys import key_set, quirk_keys
    first, again = quirk_keys()
    deltas, outs = _run(check_exe, 32, -1, [key_set(11) + first, [again]])
    assert deltas == [0, 0] and all(L["dense"] for o in outs for L in o["levels"])
    assert outs[1]["ext"][0]["E"] == 1   # the second extension for A's stem


def test_key32_extension_stage_in_parts(check_exe):
    """600 random keys: the extension stage is above its 64-row / 16,384-non-zero threshold and is
    built in several parts on the 4-worker pool (one on the 1-worker pool), with the same result; an
    update round of 300 more keys dirties more than 64 level-1 nodes, whose rows are delta rows without
    dense being forced off"""
    rng = random.Random(32)
    deltas, outs = _run(check_exe, 32, -1, [_draws(rng, 32, 256, 600), _draws(rng, 32, 256, 300)])
    assert outs[0]["ext"][0]["parts"] == 4 and outs[0]["ext"][0]["E"] == 600
    assert max(L["B"] for L in outs[0]["levels"]) > 64 and deltas[0] == 0
    assert max(L["B"] for L in outs[1]["levels"]) > 64 and deltas[1] > 64
