"""CPU: the four training libraries answer on the host exactly what tests/golden/train_host_contract.json recorded before
their argument checks were stated once with the library's name passed in: every workspace size, every return code and every
message, prefix included, byte for byte (tests/train_host_contract.py).  The host tests of each library look only for a
word in the message."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_host_contract as hc  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "train_host_contract.json")))


def test_workspace_sizes_and_refusal_messages_are_the_recorded_ones():
    got = hc.collect()
    assert set(got) == set(GOLDEN) == {"libmctrain.so", "libmctrainslow.so", "libmctrainmb.so", "libmctrainmbslow.so"}
    for name, want in GOLDEN.items():
        assert got[name]["workspace_bytes"] == want["workspace_bytes"], name
        assert set(got[name]["refusals"]) == set(want["refusals"]), name
        for what, (rc, message) in want["refusals"].items():
            assert rc == -22 and message, (name, what)
            assert got[name]["refusals"][what] == [rc, message], (name, what, got[name]["refusals"][what], message)
