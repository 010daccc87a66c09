"""The engine-free entries of the C ABI (stereo-depth_amd/csrc/smx_maps.hip) refuse what they refused, word for word.

tests/golden/map_entry_refusals.json was recorded by tools/record_map_entry_refusals.py (which documents the encoding) from
the library as it was before the entries' argument rules were gathered into shared helpers: for each of the 17 entries a
valid call, every rule broken alone, every adjacent pair of rules broken together (the order of the rules decides which
message a doubly wrong call gets), and every size query at and around its limits.  The replay requires the same status and
the same smx_last_error() text, byte for byte, and the same value of every query.

All of these checks run before a device is selected, and the pointers in the file are invented.  Without a GPU a call that
passes every check stops at "cannot select HIP device 0" and touches nothing; with one it would launch kernels on those
addresses, so the replay runs only where no HIP device is visible."""
import collections
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_entry_refusals.json")
INVALID_ARG, ERR_HIP = -1, -3
CTYPES = {"f32": C.c_float, "u16": C.c_uint16}


@pytest.fixture(scope="module")
def native():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: an accepted call would launch kernels on the file's invented addresses")
    from cuda_depth import _native
    return _native


@pytest.fixture(scope="module")
def records():
    with open(GOLDEN) as f:
        return json.load(f)


def to_c(v, keep):
    if isinstance(v, dict):
        arr = (CTYPES[v["t"]] * v["n"])(*([v["fill"]] * v["n"]))
        for k, x in v["at"]:
            arr[k] = float(x) if v["t"] == "f32" else x
        keep.append(arr)
        return arr
    return float(v) if isinstance(v, str) else v


def test_the_file_covers_every_entry_and_query(records):
    calls = collections.Counter(r["entry"] for r in records if "status" in r)
    queries = collections.Counter(r["entry"] for r in records if "value" in r)
    assert len(calls) == 17 and len(queries) == 9, (sorted(calls), sorted(queries))
    assert all(v >= 8 for v in queries.values()), queries
    for name in calls:
        statuses = [r["status"] for r in records if r["entry"] == name and "status" in r]
        assert statuses.count(ERR_HIP) == 1 and statuses.count(INVALID_ARG) == len(statuses) - 1 >= 6, (name, statuses)


def test_size_queries_return_what_they_returned(native, records):
    bad = []
    for r in records:
        if "value" in r:
            got = int(getattr(native.LIB, r["entry"])(*r["args"]))
            if got != r["value"]:
                bad.append(f"{r['entry']}{tuple(r['args'])} = {got}, recorded {r['value']}")
    assert not bad, f"{len(bad)} size queries moved:\n" + "\n".join(bad[:40])


def test_calls_are_refused_with_the_recorded_status_and_text(native, records):
    bad, calls = [], 0
    for r in records:
        if "status" not in r:
            continue
        assert len(r["args"]) == len(native.EXPORTS[r["entry"]][1]), r["entry"]
        keep = []
        rc = getattr(native.LIB, r["entry"])(*[to_c(v, keep) for v in r["args"]])
        msg = native.last_error()
        calls += 1
        if (rc, msg) != (r["status"], r["message"]):
            bad.append(f"{r['entry']}: status {rc} '{msg}'\n    recorded {r['status']} '{r['message']}'")
    assert calls >= 600
    assert not bad, f"{len(bad)} of {calls} calls answer differently:\n" + "\n".join(bad[:40])
