"""Every refusal of the entry points on top of PairRun, replayed: tests/refusals_recorded.json was recorded by
scripts/record_refusals.py from the library as it was BEFORE the entries' checks moved into csrc/density_args.hpp, and each
bad call of that table must still return its code and leave its words in kdehip_last_error().  A row marked "reordered" has
two faults of the same code whose checks changed places: its code is compared, its words may be either check's.

The rows that read a resident handle need a GPU (the handles are real; every call returns before anything is launched)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "refusals_recorded.json")))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_refusals", os.path.join(ROOT, "scripts", "record_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _replay(resident):
    want = {(r["entry"], r["case"]): r for r in TABLE if r["resident"] == resident}
    got = {(r["entry"], r["case"]): r for r in _recorder().record(resident)}
    assert sorted(got) == sorted(want)  # the list of bad calls is the recorded one
    bad = []
    for key, w in want.items():
        g = got[key]
        if g["code"] != w["code"] or (g["message"] != w["message"] and not w.get("reordered")):
            bad.append((key, (w["code"], w["message"]), (g["code"], g["message"])))
    assert not bad, bad
    return want


def test_the_table_is_what_the_issue_asks_for():
    assert all(r["code"] != 0 for r in TABLE)
    assert sum(1 for r in TABLE if not r["resident"]) > 200 and sum(1 for r in TABLE if r["resident"]) > 100
    assert sum(1 for r in TABLE if r.get("reordered")) < 0.05 * len(TABLE)


def test_host_refusals_are_the_recorded_ones():
    _replay(False)


@pytest.mark.gpu
def test_resident_refusals_are_the_recorded_ones():
    _replay(True)
