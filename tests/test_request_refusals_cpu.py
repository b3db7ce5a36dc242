"""The order of the request checks of `MMFMIL.forward`, `forward_videos`, `forward_videos_host` and `harness.score_loader`, pinned as a
whole: the enumeration of tests/request_cases.py is run on the working tree and every case must end in the exception type and the FULL
message that tests/request_refusals.json records.

The file was recorded from the commit named in its "parent" field -- the last one before the request record (`model._Request`) -- with
    python -m tests.test_request_refusals_cpu <hash of that commit> > tests/request_refusals.json
run in a checkout of that commit to which tests/request_cases.py and this file were copied.  It is never regenerated from later code: a
later change of an error message or of the check order is a change of behaviour and edits the cases it moves by hand."""
import hashlib
import json
import os
import sys

import pytest

from tests import request_cases as RC

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "request_refusals.json")


def _ids_digest(ids):
    return hashlib.sha256("\n".join(ids).encode()).hexdigest()


def record(parent: str) -> dict:
    """Each distinct (type, message) once, and per group the index of every case's outcome in the enumeration's order."""
    messages, groups = [], {}
    for group in RC.GROUPS:
        got = RC.run(group)
        for _, o in got:
            if o not in messages:
                messages.append(o)
        groups[group] = {"count": len(got), "ids_sha256": _ids_digest([cid for cid, _ in got]), "outcome": [messages.index(o) for _, o in got]}
    return {"parent": parent, "messages": messages, "groups": groups}


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_the_file_names_its_parent_and_every_group(expected):
    assert len(expected["parent"]) == 40 and set(expected["groups"]) == set(RC.GROUPS)
    # the outcomes the enumeration must reach at all: refusals of both kinds, the device check behind them, a walk that returns
    kinds = {m[0] for m in expected["messages"]}
    assert {"ValueError", "RuntimeError", "returned", "_ReachedTheWalk"} <= kinds
    assert any("runs on a HIP device only" in m[1] for m in expected["messages"])


@pytest.mark.parametrize("group", list(RC.GROUPS))
def test_every_case_ends_as_recorded(expected, group):
    want = expected["groups"][group]
    got = RC.run(group)
    assert len(got) == want["count"] and _ids_digest([cid for cid, _ in got]) == want["ids_sha256"], "the enumeration itself changed"
    wrong = [(cid, o, expected["messages"][i]) for (cid, o), i in zip(got, want["outcome"]) if o != expected["messages"][i]]
    for cid, o, w in wrong[:20]:
        print(f"{cid}\n    got      {o}\n    recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases end differently; the first: {wrong[0]}"


if __name__ == "__main__":
    rec = record(sys.argv[1])      # one message per line, one line per group
    lines = ",\n".join(json.dumps(m) for m in rec["messages"])
    groups = ",\n".join(f"{json.dumps(g)}: {json.dumps(v, separators=(',', ':'))}" for g, v in rec["groups"].items())
    sys.stdout.write(f'{{"parent": {json.dumps(rec["parent"])},\n"messages": [\n{lines}\n],\n"groups": {{\n{groups}\n}}}}\n')
