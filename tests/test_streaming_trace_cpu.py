"""The depthwise / grouped streaming-conv wrappers of ``ops`` hand the C-ABI the argument lists, and raise the errors, that were
recorded BEFORE the two families' wrappers were folded into one body per operation (tests/golden/streaming_call_trace_v1.json, made
by tests/_streaming_cases.py on that commit), and the pure shape predicates keep their values.  Runs without a device: the tensors
are CPU stand-ins that say ``is_cuda`` and no entry point is entered (tests/test_gpu_streaming_trace.py runs the calls for real)."""
import json
import os

import pytest

import _streaming_cases as SC
from pytorch_quantize_impls_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_call_trace_v1.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, "r", encoding="utf-8") as fh:
        return json.load(fh)


def test_the_recorded_cases_are_the_listed_cases(golden):
    assert sorted(golden["calls"]) == sorted(SC.CASES)
    assert sorted(golden["predicates"]) == sorted({repr(a) for a in SC.PREDICATE_CASES})     # the tables overlap
    empty = [n for n in SC.CASES if n.endswith(".empty")]
    assert len(empty) >= 16 and all(golden["calls"][n] == [] for n in empty)                # an empty batch makes no call
    refused = [n for n in SC.CASES if ".refuse." in n]
    assert refused and all(isinstance(golden["calls"][n], dict) for n in refused)
    assert all(isinstance(golden["calls"][n], list) for n in SC.CASES if ".refuse." not in n)


@pytest.mark.parametrize("family", ["dw", "gc"])
def test_wrappers_make_the_recorded_calls(golden, family):
    names = [n for n in SC.CASES if n.startswith(family + ".")]
    got = json.loads(json.dumps(SC.record_calls(None, names)))          # tuples -> lists, as the file has them
    for n in names:
        assert got[n] == golden["calls"][n], n


def test_predicates_keep_their_values(golden):
    assert SC.record_predicates() == golden["predicates"]


def test_depthwise_is_grouped_with_one_channel_per_group():
    for a in SC.PREDICATE_CASES:
        x_shape, w_shape, groups = a[0], a[1], a[5]
        one = len(x_shape) == 4 and len(w_shape) == 4 and int(groups) == int(x_shape[1]) and int(w_shape[1]) == 1
        assert ops.depthwise_applicable(*a) == bool(one and ops.grouped_applicable(*a)), a
