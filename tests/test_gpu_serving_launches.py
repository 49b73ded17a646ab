"""The serving entries launch what they launched and return the bits they returned when tests/golden/serving_launches.json was recorded
(tools/record_serving_launches.py, at the commit before the serving path was described once): per case the timing hook's (role, kernel, launches)
list is equal -- same kernels, same counts, nothing extra -- and so is the SHA-256 of every returned tensor.  Together with identical device code
(tools/isa_diff.py) that is the evidence that a host-side refactor left the device's work alone."""
import json
import os

import pytest

import serving_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "serving_launches.json")


@pytest.mark.parametrize("hm,setting", SC.GROUPS, ids=[SC.group_id(*g) for g in SC.GROUPS])
def test_serving_cases_launch_and_return_what_was_recorded(hm, setting):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert (golden["batch"], golden["hm_chunk"]) == (SC.B, SC.CHUNK)
    got = SC.run_group(hm, setting)
    want = {cid: c for cid, c in golden["cases"].items() if cid.startswith(SC.group_id(hm, setting) + "/")}
    assert sorted(got) == sorted(want) and len(got) == len(SC.ENTRIES) * len(SC.OUTPUTS)
    wrong = []
    for cid, (launches, hashes) in got.items():
        recorded = [golden["kernels"][k] + [n] for k, n in golden["launch_lists"][want[cid]["launches"]]]
        if launches != recorded:
            wrong.append((cid, "launches", launches, recorded))
        if cid not in golden["unstable"] and hashes != want[cid]["sha256"]:
            wrong.append((cid, "sha256", hashes, want[cid]["sha256"]))
    assert not wrong, wrong
