"""The sequence harness of oracle/handle_model.py without a GPU: the proof that
it would notice.

* Plumbing: the model wrapped as a fake handle (and as a fake group of strips)
  runs every committed (configuration, seed) against the model and passes.
* Mutants: for each one-line defect of the fake, at least one committed
  sequence raises SequenceMismatch within its 40 calls.  The defects are the
  fake's; nothing here runs a kernel.
* Call-kind coverage: the committed seeds draw every call kind of their tables
  at least twice, and at least one job in flight has a stamp, a clear and a
  step between its begin and its wait; over the "-rules" seeds a stamp_file was
  refused for its rule and one accepted (one of a file the sequence saved), a
  save_rle refused on an empty board, and split_rule made all seven group calls.
* The first thirty sequences do not move: the calls they draw are pinned by the
  digests of tests/golden/sequence_lines_parent.json, written from the tree as
  it was before the "-rules" tables came (tests/golden/make_sequence_lines.py).
"""
import ast
import hashlib
import json
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
    "128x17-rules": [1, 2, 45],
    "192x33-rules": [1, 45, 390],
    "100x37-rules": [45, 146, 227],
    "33x9-rules": [1, 2, 7],
    "128x130-rules": [1, 2, 147],
    "128x50-strips-rules": [35, 98, 185],
    "100x50-strips-rules": [38, 66, 101],
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
    # ... and of the Life-like rules and the pattern savers
    "rule_lags_a_call",           # the first stepping call after set_rule still runs the old rule
    "stream_steps_conway",        # flip streams ignore the rule
    "set_rule_drops_flips",       # flips() refused after set_rule
    "extract_drops_flips",        # an observer that invalidates the kept list
    "extract_no_x_wrap",          # an extract without its second column segment
    "box_not_cyclic",             # the alive box as min..max per axis, not the shortest cyclic interval
    "rle_names_conway",           # save_rle always writing Conway's rule
    "stamp_file_any_rule",        # a file of another rule accepted
    "split_rule_steps",           # a group with one strip on another rule steps anyway
    "rule_stream_keeps_flips",    # a group's flip stream under a rule that leaves flips() served (finding 3)
]
GROUP_DEFECTS = ("strip_behind", "split_rule_steps", "rule_stream_keeps_flips")  # defects of the fake group


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


NEW_DEFECTS = DEFECTS[10:]  # each must be caught by a sequence of the "-rules" configurations


def caught_by(defect, tmp_path_factory):
    for name, seed in CASES:
        if defect in NEW_DEFECTS and hm.CONFIGS[name].get("table") != "rules":
            continue
        if defect in GROUP_DEFECTS and hm.CONFIGS[name].get("cuts") is None:
            continue
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
    for key, tables in hm.TABLES.items():
        for group, table in ((False, tables[0]), (True, tables[1])):
            drawn: dict = {}
            for name in SEEDS:
                if hm.config_table(name) is table:
                    for k, n in stats[name]["kinds"].items():
                        drawn[k] = drawn.get(k, 0) + n
            few = {k: drawn.get(k, 0) for k in hm.table_kinds(table) if drawn.get(k, 0) < 2}
            assert not few, f"{key} {'group' if group else 'torus'} table kinds drawn fewer than twice: {few}"
    assert any({"stamp", "clear", "step"} <= s for st in stats.values() for s in st["jobs_between"])
    notes = set().union(*(st["notes"] for name, st in stats.items() if hm.CONFIGS[name].get("table") == "rules"))
    assert {"stamp_file_refused_for_its_rule", "stamp_file_accepted", "save_rle_empty"} <= notes, notes
    # a file an earlier save_rle of the sequence wrote went back through stamp_file and was taken
    assert "stamp_file_saved_accepted" in notes, notes
    # split_rule made each of its seven group calls with one strip on another rule
    inner = {"step", "flip_stream", "view_frame", "stamp", "extract", "alive_box", "save_rle"}
    assert {"split_rule:" + w for w in inner} <= notes, sorted(n for n in notes if n.startswith("split_rule:"))


def test_old_sequences_unchanged(tmp_path_factory):
    """The thirty sequences committed before the "-rules" tables draw the calls
    they drew then: the digests were written by the parent's code."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "sequence_lines_parent.json")) as f:
        pinned = json.load(f)
    old = [(name, seed) for name, seed in CASES if hm.CONFIGS[name].get("table") is None]
    assert sorted(pinned) == sorted(f"{name}:{seed}" for name, seed in old) and len(old) == 30
    for name, seed in old:
        tmp = tmp_path_factory.mktemp("d")
        d = hm.run_config(name, seed, tmp, target=fake(name))
        text = "\n".join(d.lines).replace(str(tmp), "<TMP>")
        assert hashlib.sha256(text.encode()).hexdigest() == pinned[f"{name}:{seed}"], (name, seed)
