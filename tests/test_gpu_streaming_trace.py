"""tests/test_streaming_trace_cpu.py on the device: the same list of calls into the depthwise / grouped streaming-conv wrappers, on
real device tensors and with every entry point entered, makes the argument lists and raises the errors recorded before the two
families' wrappers were folded into one body per operation (tests/golden/streaming_call_trace_v1.json)."""
import json
import os

import pytest
import torch

import _streaming_cases as SC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_call_trace_v1.json")


@pytest.mark.parametrize("family", ["dw", "gc"])
def test_wrappers_make_the_recorded_calls_on_the_device(family):
    with open(GOLDEN, "r", encoding="utf-8") as fh:
        golden = json.load(fh)["calls"]
    names = [n for n in SC.CASES if n.startswith(family + ".")]
    got = json.loads(json.dumps(SC.record_calls(torch.device("cuda:0"), names)))
    torch.cuda.synchronize()
    for n in names:
        assert got[n] == golden[n], n
