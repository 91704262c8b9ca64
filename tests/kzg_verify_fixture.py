"""Test helper: tests/golden/kzg_verify_16.json (tests/golden/make_kzg_verify_golden.py) as
Python values. Entries are dicts with commitment / proof as (x, y) | None, point and y as ints,
and `valid`, the oracle's verdict (protocol.KZG.verify_point)."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _pt(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


def load():
    with open(os.path.join(HERE, "golden", "kzg_verify_16.json")) as f:
        g = json.load(f)
    g2 = tuple(tuple(int(v, 16) for v in c) for c in g["g2"])
    entries = [{"name": e["name"], "commitment": _pt(e["commitment"]), "point": int(e["point"], 16),
                "proof": {"proof": _pt(e["proof"]), "y": int(e["y"], 16)}, "valid": e["valid"]}
               for e in g["entries"]]
    return {"secret": g["secret"], "size": g["size"], "g2": g2, "entries": entries,
            "data": [int(v, 16) for v in g["data"]]}
