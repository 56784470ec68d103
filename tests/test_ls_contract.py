"""The C ABI of the layer-synchronous engine answers bad arguments as it did when tests/golden/ls_contract.json was recorded
(tools/record_ls_contract.py, section "abi"): every case fails a validation check, so it returns before any HIP call and needs no GPU."""
import importlib.util
import json
import os

from conftest import GOLDEN, REPO


def load_recorder():
    spec = importlib.util.spec_from_file_location("record_ls_contract", os.path.join(REPO, "tools", "record_ls_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_contract():
    with open(os.path.join(GOLDEN, "ls_contract.json")) as fh:
        return json.load(fh)


def test_abi_return_codes_match_the_record():
    want = load_contract()["abi"]
    got = load_recorder().run_abi()
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_the_record_covers_every_ls_entry_point():
    """a new LS entry point in _lib.SIGNATURES has to be added to the recorder's tables (and recorded)"""
    from nerf_atlas_amd import _lib
    rec = load_recorder()
    ls_entries = {n for n in _lib.SIGNATURES if n.endswith(("_ls", "_ls_pack", "_ls_rayts"))}
    assert ls_entries == set(rec.RENDERS) | set(rec.PACKS), ls_entries ^ (set(rec.RENDERS) | set(rec.PACKS))
    want = load_contract()["abi"]
    for name in ls_entries:
        assert any(k.startswith(name + "/") for k in want), name
