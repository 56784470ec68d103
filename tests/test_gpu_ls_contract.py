"""Every weight stream and every output of the layer-synchronous engine is byte for byte what it was when
tests/golden/ls_contract.json was recorded (tools/record_ls_contract.py, sections "pack" and "render"): the host path in front of
the kernels (csrc/render_ls.hip, csrc/ls_pack.h) can be rearranged, what reaches the GPU cannot change unnoticed."""
import pytest

from test_ls_contract import load_contract, load_recorder

pytestmark = pytest.mark.gpu


def _compare(got, want):
    assert set(got) == set(want), sorted(set(got) ^ set(want))  # a missing case fails
    diff = sorted(k for k in want if got[k] != want[k])
    assert not diff, diff


def test_pack_streams_match_the_record():
    c = load_contract()
    _compare(load_recorder().run_pack(c["shift"]), c["pack"])


def test_render_outputs_match_the_record():
    c = load_contract()
    assert c["unstable"] == [], c["unstable"]  # (every case was bit-reproducible when recorded: all of them are compared exactly)
    _compare(load_recorder().run_render(c["shift"]), c["render"])
