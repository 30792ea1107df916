"""Issue order of the deferred-store kernel's loads, read from the gfx950 ISA of
the BUILT libdlsim_hip.so (CPU test; scripts/audit_isa.py extracts and
disassembles the code objects).

Every k_wreduce_defer_pre<F32Exact, ..., NF, ..., RC> compiled for its row
count (RC > 0) folds its RC rows in one straight-line block: RC * NF
global_load_dwordx4. Up to R = 24 the source reads each group of two rows in
bursts of two inputs (wreduce_kernels.hpp defer_burst), each burst pinned
between scheduling barriers and folded before the next issues. The barriers
leave no instruction behind, so here a burst is the next run of that many
loads of the block. (Above R = 24 a group is one burst left to the scheduler,
on measurement; these checks do not cover it.)

* No `s_waitcnt vmcnt` sits between the first and the last load of a burst.
  Loads return in order, so such a wait is a memory round trip the source did
  not ask for, with part of the burst in flight. (Before the bursts were
  pinned the scheduler hoisted the fold's x0 * 0 seed between the loads of
  what the source wrote as one burst of 16: 10 of the 11 row groups of NF 8,
  RC 22 were split; test_detector_counts_split_bursts.)
* Every burst is waited for before the next one issues: the fold, not the
  scheduler, decides what is in flight.
* No deferred kernel uses scratch or more than 256 VGPRs (a 512-lane block has
  256 per lane).
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import audit_isa  # noqa: E402

NAME_RE = re.compile(r"k_wreduce_defer_pre.*8F32Exact.*EELi(\d+)ELi8ELi(\d+)ELi2ELi2ELi(\d+)EE")
BRANCH_RE = re.compile(r"^\s*(s_cbranch\w*|s_branch|s_endpgm|s_setpc_b64)\b")
LOAD_RE = re.compile(r"^\s*global_load_dwordx4\b")
WAIT_RE = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")


def events(body):
    """The straight-line block of `body` with the most 16-byte loads, from its
    first load on, as a list of "L" (a load) and integers (the count an
    s_waitcnt vmcnt leaves outstanding). (The listing has no labels: the
    scalar tail's masked code, which falls through into a last block's rows,
    is what the cut before the first load removes.)"""
    blocks = [[]]
    for line in body.splitlines():
        if BRANCH_RE.match(line):
            blocks.append([])
        elif LOAD_RE.match(line):
            blocks[-1].append("L")
        else:
            m = WAIT_RE.match(line)
            if m:
                blocks[-1].append(int(m.group(1)))
    best = max(blocks, key=lambda b: b.count("L"))
    return best[best.index("L"):] if "L" in best else best


def bursts(nf, rc):
    """Loads per burst, in issue order (defer_burst: two inputs x two rows)."""
    assert rc <= 24
    return ([4] * (nf // 2) + [2] * (nf % 2)) * (rc // 2)


def split_bursts(ev, sizes):
    """How many of the consecutive runs of sizes[k] loads hold a wait."""
    bad, seen, k, waited = 0, 0, 0, False
    for e in ev:
        if e == "L":
            seen += 1
            if seen == sizes[k]:
                bad += waited
                seen, k, waited = 0, k + 1, False
        elif seen:
            waited = True
    assert k == len(sizes) and seen == 0, "the block's loads are not these bursts"
    return bad


def unwaited(ev, sizes):
    """How many bursts the next burst follows without a wait to zero."""
    bad, seen, k, zero = 0, 0, 0, True
    for e in ev:
        if e == "L":
            if seen == 0:
                bad += not zero
            zero = False
            seen += 1
            if seen == sizes[k]:
                seen, k = 0, k + 1
        elif e == 0:
            zero = True
    return bad


@pytest.fixture(scope="module")
def deferred():
    """{(NF, RC): events} of the exact policy's compiled-R deferred kernels."""
    if not os.path.exists(audit_isa.LIB):
        pytest.fail("libdlsim_hip.so is not built (run __graft_entry__.build())")
    out = {}
    for co in audit_isa.code_objects(audit_isa.LIB):
        if b"k_wreduce_defer_pre" not in co or b"8F32Exact" not in co:
            continue  # (disassembling a unit takes seconds)
        for name, body in audit_isa.kernels(audit_isa.disassemble(co)).items():
            m = NAME_RE.search(name)
            if m and int(m.group(3)) > 0:
                out[(int(m.group(1)), int(m.group(3)))] = events(body)
    return out


def test_every_compiled_row_count_is_read(deferred):
    assert len(deferred) == 168 and (8, 22) in deferred
    for (nf, rc), ev in deferred.items():
        assert ev.count("L") == nf * rc, (nf, rc, ev.count("L"))


def test_no_wait_inside_a_burst(deferred):
    bad = {k: split_bursts(ev, bursts(*k)) for k, ev in deferred.items() if k[1] <= 24}
    assert len(bad) == 132 and not any(bad.values()), {k: v for k, v in bad.items() if v}


def test_every_burst_is_folded_before_the_next_issues(deferred):
    bad = {k: unwaited(ev, bursts(*k)) for k, ev in deferred.items() if k[1] <= 24}
    assert len(bad) == 132 and not any(bad.values()), {k: v for k, v in bad.items() if v}


def test_detector_counts_split_bursts():
    """The shapes the detector must tell apart, NF = 8, RC = 22. What the
    compiler made of the flagship's row groups when the source wrote them as
    one burst of 16 (2 loads, a wait, 14 loads, the fold's ladder): 10 split
    bursts of 16. The shipped form (4 loads, their fold, 4 loads): none."""
    ladder = list(range(15, -1, -1))
    before = ["L"] * 16 + ladder + (["L"] * 2 + [1] + ["L"] * 14 + ladder) * 6 + \
        (["L"] * 9 + [8] + ["L"] * 7 + ladder) * 3 + ["L"] * 12 + [1] + ["L"] * 4 + [3, 2, 1, 0]
    assert before.count("L") == 8 * 22 and split_bursts(before, [16] * 11) == 10
    with pytest.raises(AssertionError):
        split_bursts(before[:-8], [16] * 11)
    now = (["L"] * 4 + [3, 1, 0]) * 44
    assert bursts(8, 22) == [4] * 44 and split_bursts(now, bursts(8, 22)) == 0 and unwaited(now, bursts(8, 22)) == 0
    assert bursts(3, 6) == [4, 2] * 3
    rolling = ["L"] * 8 + ([7, 5, 4] + ["L"] * 4) * 42 + [3, 1, 0]
    assert split_bursts(rolling, bursts(8, 22)) == 0 and unwaited(rolling, bursts(8, 22)) == 43


def test_deferred_kernels_fit_their_registers():
    """Kernel metadata of the library: every deferred kernel (512 lanes: one
    block per CU, 256 VGPRs per lane) has no scratch and fits."""
    seen = 0
    for co in audit_isa.code_objects(audit_isa.LIB):
        with audit_isa.tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "co.elf")
            with open(p, "wb") as f:
                f.write(co)
            notes = subprocess.run([os.path.join(audit_isa.LLVM, "llvm-readelf"), "--notes", p], check=True,
                                   capture_output=True, text=True).stdout
        for k in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", k).group(1)
            if "k_wreduce_defer" not in name:
                continue
            seen += 1
            agpr = int(k.split()[0])
            vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", k).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1))
            assert scratch == 0 and max(vgpr, agpr + vgpr) <= 256, (name, vgpr, agpr, scratch)
    assert seen >= 168
