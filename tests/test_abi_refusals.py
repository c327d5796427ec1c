"""Every refusal of the measure, annotate, overlay and JPEG-encode entry points, and of the frame-table and window-table path (pack,
table readers, letterbox, scale_boxes, ragged native masks, the table predicts), answers as it did at the commit recorded in
tests/golden/abi_refusals.json: the same status and, byte for byte, the same message.  The cases (tests/abi_refusal_cases.py) are
refused calls only, built from fake pointers that are never dereferenced, so nothing is launched wherever this runs."""
import json
import os

import pytest

from abi_refusal_cases import cases

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")))


@pytest.fixture(scope="module")
def calls(lib_built):
    return {(entry, case): call for entry, case, call in cases(lib_built)}


def test_the_record_and_the_cases_name_the_same_calls(calls):
    recorded = [(entry, case) for entry, case, _, _ in RECORD["rows"]]
    assert len(recorded) == len(set(recorded)) >= 1007 and set(recorded) == set(calls)
    assert len(RECORD["commit"]) == 40


@pytest.mark.parametrize("entry", sorted({row[0] for row in RECORD["rows"]}))
def test_every_refusal_answers_as_recorded(calls, entry):
    rows = [row for row in RECORD["rows"] if row[0] == entry]
    assert rows
    for _, case, status, message in rows:
        assert calls[(entry, case)]() == (status, message), (entry, case)
