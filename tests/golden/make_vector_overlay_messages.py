"""Record what the reference's ``viewer_contract.vector_overlay_vertices`` answers to a list of inputs:
tests/golden/vector_overlay_messages.json, the fixture ViewerHandle.add_vector_overlay's validation is held to
(tests/test_session_paint_host.py).

    python tests/golden/make_vector_overlay_messages.py <checkout of the reference>

The function is pure Python; it is imported from the checkout, called, and only its answers are written: per case the input
rows, and either the message of the ValueError it raised or the rows it returned.
"""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "vector_overlay_messages.json"
GOOD = [0.0, 1.0, 2.0, 0.1, 0.2, 0.3, 1.0, 7]


def cases():
    def row(**lanes):
        r = list(GOOD)
        for k, v in lanes.items():
            r[int(k[1:])] = v
        return r

    return [
        ("one good row", [GOOD]),
        ("two good rows, ids as float and int", [GOOD, row(_7=4294967295), row(_7=3.0)]),
        ("seven lanes", [GOOD[:7]]),
        ("nine lanes", [GOOD + [0]]),
        ("second row short", [GOOD, GOOD[:3]]),
        ("x is nan", [row(_0="nan")]),
        ("y is inf", [row(_1="inf")]),
        ("z is -inf", [GOOD, row(_2="-inf")]),
        ("red above one", [row(_3=1.5)]),
        ("alpha negative", [row(_6=-0.01)]),
        ("green is nan", [row(_4="nan")]),
        ("id is a bool", [row(_7=True)]),
        ("id is a fraction", [row(_7=1.5)]),
        ("id is negative", [row(_7=-1)]),
        ("id is 2^32", [row(_7=4294967296)]),
        ("id is text", [row(_7="road")]),
        ("id is None", [row(_7=None)]),
        ("id is nan", [row(_7="nan")]),
        ("empty list", []),
    ]


def decode(rows):
    """JSON has no nan / inf: they are written as text in lanes 0..6 and turned back into floats here (and in the test)."""
    return [[float(v) if isinstance(v, str) and i < 7 else (float(v) if v == "nan" else v) for i, v in enumerate(r)] for r in rows]


def main(reference: Path) -> None:
    spec = importlib.util.spec_from_file_location("viewer_contract", reference / "python" / "forge3d" / "viewer_contract.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = []
    for name, rows in cases():
        entry = {"name": name, "vertices": rows}
        try:
            entry["returns"] = module.vector_overlay_vertices(decode(rows))
        except ValueError as exc:
            entry["message"] = str(exc)
        out.append(entry)
    OUT.write_text(json.dumps({"function": "viewer_contract.vector_overlay_vertices", "cases": out}, indent=1) + "\n")
    print(f"{OUT}: {len(out)} cases, {sum('message' in e for e in out)} refusals")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
