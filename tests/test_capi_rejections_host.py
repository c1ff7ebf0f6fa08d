"""Every streamed entry point of the C-ABI (an scr_* function of include/splatco_raster.h whose last parameter is
`void* stream`) against tests/golden/capi_rejections.json: the status and the scr_last_error() text it gave, before it
launched anything, to the synthetic argument vectors of tools/make_golden_rejections.py (all pointers NULL or one zeroed
host buffer; all integers 1, -1 or 0).  An argument check that is lost, reordered or reworded fails here without a device.

Skipped where a device is present: a lost NULL check would there become a launch on made-up pointers."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_rejections as gen  # noqa: E402

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")


@pytest.fixture(scope="module")
def table():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_table_names_every_streamed_entry_point(table):
    from splatco_amd import _C
    streamed = gen.streamed_entry_points()
    assert len(streamed) > 50 and set(streamed) <= set(_C.SYMBOLS)
    assert "scr_flip_filters" not in streamed and "scr_geom_bytes" not in streamed
    assert {r["name"] for r in table} == set(streamed)
    assert {r["vector"] for r in table} == set(gen.VECTORS)
    # what the table may hold: returns from before a launch, and for every function at least one refusal with its reason
    assert all(gen.before_launch(r["rc"], r["error"]) and (r["rc"] != 0) == bool(r["error"]) for r in table)
    assert {r["name"] for r in table if r["rc"] != 0} == set(streamed)


def test_every_recorded_case_gets_the_same_status_and_message(table):
    from splatco_amd import _C
    buf = gen.Buffer()
    wrong = []
    for r in table:
        rc, message = gen.run_case(_C, r["name"], r["vector"], buf)
        if (rc, message) != (r["rc"], r["error"]):
            wrong.append(f'{r["name"]} {r["vector"]}: {rc} "{message}", recorded {r["rc"]} "{r["error"]}"')
    assert not wrong, "\n".join(wrong)
