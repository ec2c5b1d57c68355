"""The sequence harness of oracle/handle_model.py without a GPU: the proof that
it would notice.

* Plumbing: the model wrapped as a fake handle (and as a fake group of strips)
  runs every committed (configuration, seed) against the model and passes.
* Mutants: for each one-line defect of the fake, at least one committed
  sequence raises SequenceMismatch within its 40 calls.  The defects are the
  fake's; nothing here runs a kernel.
* Call-kind coverage: the committed seeds draw every call kind of the two
  tables at least twice, and at least one job in flight has a stamp, a clear
  and a step between its begin and its wait.
"""
import ast
import os

import pytest

import oracle.handle_model as hm

# the seeds of tests/test_gpu_sequences.py (test_seeds_match_the_gpu_suite)
SEEDS = {
    "128x17": [13, 29, 34],
    "256x40": [14, 15, 16],
    "192x33": [2, 27, 37],
    "96x20": [11, 21, 23],
    "100x37": [1, 10, 11],
    "33x9": [9, 11, 18],
    "5x3": [13, 25, 37],
    "128x130": [28, 29, 30],
    "128x50-strips": [10, 20, 21],
    "100x50-strips": [1, 12, 23],
}
CASES = [(name, seed) for name, seeds in SEEDS.items() for seed in seeds]

DEFECTS = [
    "count_kept_over_stamp",      # the alive count not invalidated by a stamp
    "flips_kept_over_stamp",      # flips() still served after a stamp
    "clear_keeps_turn",           # clear not resetting the turn
    "stamp_drops_columns",        # a stamp dropping its second column segment
    "stamp_drops_rows",           # a stamp dropping its second row interval
    "shadow_sees_later_edits",    # a checkpoint or image shadow that sees a later stamp
    "stream_advances_on_erange",  # a flip stream that advances on ERANGE
    "stream_drops_last",          # a flip stream that drops the last entry of a stopped batch
    "padding_bit_set",            # snapshot_bits with a padding bit set
    "strip_behind",               # one strip left a turn behind after a stopped group stream
]

def fake(name, defect=None):
    c = hm.CONFIGS[name]
    return hm.HandleModel(c["W"], c["H"], c.get("cuts"), fake=True, defect=defect)


def test_seeds_match_the_gpu_suite():
    path = os.path.join(os.path.dirname(__file__), "test_gpu_sequences.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    found = [ast.literal_eval(n.value) for n in tree.body
             if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "SEEDS"]
    assert found == [SEEDS]
    assert set(SEEDS) == set(hm.CONFIGS) and all(len(s) == 3 for s in SEEDS.values())


@pytest.mark.parametrize("name,seed", CASES)
def test_model_against_model(name, seed, tmp_path):
    """Plumbing: a faithful fake passes."""
    hm.run_config(name, seed, tmp_path, target=fake(name))


def caught_by(defect, tmp_path_factory):
    for name, seed in CASES:
        if defect == "strip_behind" and hm.CONFIGS[name].get("cuts") is None:
            continue  # (a defect of the fake group)
        try:
            hm.run_config(name, seed, tmp_path_factory.mktemp("m"), target=fake(name, defect))
        except hm.SequenceMismatch as e:
            return name, seed, e
    return None


@pytest.mark.parametrize("defect", DEFECTS)
def test_mutant_is_caught(defect, tmp_path_factory):
    hit = caught_by(defect, tmp_path_factory)
    assert hit is not None, f"no committed sequence notices the defect {defect}"
    name, seed, e = hit
    # the calls so far replay as pasted: on a fresh fake with the same defect the
    # block runs to its end and its last line gives the same wrong answer
    assert e.lines[1] == "import oracle.handle_model as hm" and e.lines[2].startswith("t = hm.")
    assert str(e).endswith("\n".join(e.lines))
    env = {"t": fake(name, defect)}
    exec("\n".join(e.lines[1:2] + e.lines[3:-1]), env)
    again = eval(e.lines[-1].split("  #")[0], env)
    assert again[0] in ("ok", "refused")
    if e.got is not None:  # (None: the answers agreed and the job's file differed)
        assert hm.Driver.same(again, e.got), (name, seed, e.lines[-1])
    # ... and a faithful fake answers that line otherwise, or writes another file
    env = {"t": fake(name)}
    exec("\n".join(e.lines[1:2] + e.lines[3:-1]), env)
    good = eval(e.lines[-1].split("  #")[0], env)
    assert e.got is None or not hm.Driver.same(good, e.got), (name, seed, e.lines[-1])


def test_call_kind_coverage(tmp_path_factory):
    """Every kind of the tables at least twice over the committed seeds; one job
    with a stamp, a clear and a step between begin and wait."""
    stats = {name: {} for name in SEEDS}
    for name, seed in CASES:
        hm.run_config(name, seed, tmp_path_factory.mktemp("c"), target=fake(name), stats=stats[name])
    for group, table in ((False, hm.TORUS_TABLE), (True, hm.GROUP_TABLE)):
        drawn: dict = {}
        for name in SEEDS:
            if (hm.CONFIGS[name].get("cuts") is not None) == group:
                for k, n in stats[name]["kinds"].items():
                    drawn[k] = drawn.get(k, 0) + n
        few = {k: drawn.get(k, 0) for k in hm.table_kinds(table) if drawn.get(k, 0) < 2}
        assert not few, f"{'group' if group else 'torus'} table kinds drawn fewer than twice: {few}"
    assert any({"stamp", "clear", "step"} <= s for st in stats.values() for s in st["jobs_between"])
