"""The in-launch hand-off of the one-launch AUTO kernel, checked in its gfx950 assembly.

Off the exact grid, the workgroups of k_match_auto_small (k_match_auto.h) become disparity slices: each writes its partial
arg-max records with device-scope (sc1, write-through) stores, then thread 0 takes a ticket of the tile
(e2_merge_by_last_arriver, k_match_exact2.h), and the last slice to arrive merges the tile's records.  The ticket may only
be taken once every wave's records have landed: each wave drains its stores (s_waitcnt vmcnt(0)) before the barrier that
precedes the ticket atomic; an s_barrier waits for no memory counter.  Without the drain the merger can read the records
an earlier call left behind -- a race a GPU run would rarely show, so the order is checked in the code the compiler emits.
The merger reads the records with sc1 loads.  No GPU involved: tu_fast_small.hip is compiled to device assembly with
build.py's flags."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# TH (8, 10, 12) x right-tile pitch (256, 320) x packed-sum form (0, 1, 2), all launched by launch_match_auto_small
INSTANTIATIONS = 18
SLICE_WORDS = 8                      # smx_common.h: SMX_SLICE_WORDS records per pixel and slice

LABEL = re.compile(r"^(\.LBB\S*:|; %bb\.\d+:)")
BRANCH = re.compile(r"^\s*s_(c?branch|setpc|endpgm)")
STORE = re.compile(r"^\s*(global|buffer|flat|scratch)_store")
LOAD = re.compile(r"^\s*(global|buffer|flat|scratch)_load")
VMCNT0 = re.compile(r"^\s*s_waitcnt\s.*\bvmcnt\(0\)")
TICKET = re.compile(r"^\s*global_atomic_add\s.*\bsc0\b")       # the returning add: the ticket
BARRIER = re.compile(r"^\s*s_barrier\b")


def _build_module():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def auto_kernels(tmp_path_factory):
    """{symbol: [instruction lines]} of every k_match_auto_small instantiation."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    out = str(tmp_path_factory.mktemp("auto_isa") / "tu_fast_small.s")
    cmd = [b.hipcc()] + b.FLAGS + ["-I", b.INCLUDE, "--cuda-device-only", "-S", "-o", out,
                                   os.path.join(b.CSRC, "tu_fast_small.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, "hipcc -S failed:\n" + r.stdout + r.stderr
    kernels, cur = {}, None
    for ln in open(out):
        ln = ln.rstrip("\n")
        m = re.match(r"^(_ZN3smx18k_match_auto_small\w+):", ln)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is not None and (ln.startswith(".Lfunc_end") or ln.lstrip().startswith(".amdhsa_kernel")):
            cur = None
        if cur is not None:
            cur.append(ln)
    return kernels


def _ticket_sites(body):
    """(ticket atomic, barrier before it, the barrier before that) line indices of every ticket in a kernel."""
    sites = []
    for i, ln in enumerate(body):
        if TICKET.match(ln):
            bar = max((j for j in range(i) if BARRIER.match(body[j])), default=None)
            assert bar is not None, "no barrier before the ticket"
            prev = max((j for j in range(bar) if BARRIER.match(body[j])), default=-1)
            sites.append((i, bar, prev))
    return sites


def test_every_instantiation_is_found(auto_kernels):
    assert len(auto_kernels) == INSTANTIATIONS, sorted(auto_kernels)
    for sym, body in auto_kernels.items():
        assert len(_ticket_sites(body)) >= 1, f"{sym}: no ticket atomic"


def test_records_are_drained_before_the_ticket_barrier(auto_kernels):
    """In the basic block that ends at the barrier before each ticket: an s_waitcnt vmcnt(0) with no store after it.
    Every path to the barrier runs through that block, so every wave has completed its record stores when thread 0
    passes the barrier and adds to the ticket."""
    bad = []
    for sym, body in auto_kernels.items():
        for tick, bar, _ in _ticket_sites(body):
            start = bar
            while start > 0 and not LABEL.match(body[start - 1]) and not BRANCH.match(body[start - 1]):
                start -= 1
            block = body[start:bar]
            waits = [k for k, ln in enumerate(block) if VMCNT0.match(ln)]
            if not waits or any(STORE.match(ln) for ln in block[waits[-1]:]):
                bad.append(f"{sym} (ticket at line {tick}): barrier block\n  " + "\n  ".join(body[start:bar + 1]))
    assert not bad, "the ticket is taken without draining the slice records first:\n" + "\n".join(bad)


def test_ticket_branch_stores_and_merge_loads_are_device_scope(auto_kernels):
    """Records: between the two barriers before the ticket, at least one sc1 store per record word, and every plain
    store there is the tickets == NULL alternative of an sc1 store with the same operands (match_exact2_body's put).
    Merge: every vector load after the ticket carries sc1 (the records come from other workgroups, other XCDs)."""
    bad = []
    for sym, body in auto_kernels.items():
        for tick, bar, prev in _ticket_sites(body):
            stores = [ln.strip() for ln in body[prev + 1:bar] if STORE.match(ln)]
            sc1 = {s for s in stores if re.search(r"\bsc1\b", s)}
            if len(sc1) < SLICE_WORDS:
                bad.append(f"{sym}: {len(sc1)} sc1 record stores before the ticket")
            for s in stores:
                if s not in sc1 and s + " sc1" not in sc1:
                    bad.append(f"{sym}: record store without an sc1 form: {s}")
            end = next((k for k in range(tick, len(body)) if re.match(r"^\s*s_endpgm", body[k])), len(body))
            loads = [ln.strip() for ln in body[tick:end] if LOAD.match(ln)]
            if not loads:
                bad.append(f"{sym}: no merge loads after the ticket")
            bad += [f"{sym}: merge load without sc1: {ld}" for ld in loads if not re.search(r"\bsc1\b", ld)]
    assert not bad, "\n".join(bad)
