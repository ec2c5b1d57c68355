"""Writes tests/golden/sequence_lines_parent.json: one digest per committed
(configuration, seed) of the first thirty seeded call sequences (DESIGN.md
§3.3), taken model against model.

The fixture pins the calls those sequences draw, so it is generated from the
tree BEFORE a change to oracle/handle_model.py (check the parent commit out and
run this file there), never from the code under test:

    python tests/golden/make_sequence_lines.py

A digest is the SHA-256 of the driver's replay lines joined by newlines, the
temporary directory's name replaced by the token <TMP>.
tests/test_sequences_cpu.py::test_old_sequences_unchanged computes the same
from today's code.
"""
import ast
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle.handle_model as hm  # noqa: E402


def old_seeds() -> dict:
    """The seeds of tests/test_gpu_sequences.py whose configuration draws from the first tables."""
    with open(os.path.join(ROOT, "tests", "test_gpu_sequences.py")) as f:
        tree = ast.parse(f.read())
    seeds = [ast.literal_eval(n.value) for n in tree.body
             if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "SEEDS"][0]
    return {name: s for name, s in seeds.items() if hm.CONFIGS[name].get("table") is None}


def digest(lines, tmp) -> str:
    return hashlib.sha256("\n".join(lines).replace(str(tmp), "<TMP>").encode()).hexdigest()


def main():
    out = {}
    for name, seeds in old_seeds().items():
        c = hm.CONFIGS[name]
        for seed in seeds:
            with tempfile.TemporaryDirectory() as tmp:
                fake = hm.HandleModel(c["W"], c["H"], c.get("cuts"), fake=True)
                d = hm.run_config(name, seed, tmp, target=fake)
                out[f"{name}:{seed}"] = digest(d.lines, tmp)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sequence_lines_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} digests -> {path}")


if __name__ == "__main__":
    main()
