"""Where the rides of csrc/proj_ring.hip stand in the generated code.  One wave per SIMD: behind a 32-cycle matrix instruction
about five 4-cycle vector instructions issue for free and at most one 8-cycle transcendental among them; what a gap holds beyond
that is paid in full while the neighbouring gaps hide nothing.  Two design rules follow, and both are properties of the code
hipcc makes, not of the source (left alone hipcc gathered a whole query chunk's elu + 1 behind ONE matrix instruction):

  * no gap between two matrix instructions of a stage holds more than one transcendental;
  * no gap holds more than eight vector instructions (8 x 4 cycles is the matrix instruction's own duration: a fuller gap
    cannot hide even in principle).

A stage is what stands between two s_barrier of proj_ring_kernel<SplitH2> with at least 96 matrix instructions."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANS = ("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")


def _stages(body):
    """per stage: the list of (vector instructions, transcendentals) of its gaps, in program order"""
    stages, gaps, v, t, seen = [], [], 0, 0, False
    for line in body.splitlines():
        s = line.strip()
        if not s or s.startswith(";") or s.endswith(":") or re.match(r"^\.L\S+:", s):
            continue
        op = s.split()[0]
        if op == "s_barrier":
            stages.append(gaps)
            gaps, v, t, seen = [], 0, 0, False
        elif op.startswith("v_mfma"):
            if seen:
                gaps.append((v, t))
            v, t, seen = 0, 0, True
        elif op.startswith("v_"):
            v += 1
            t += op.startswith(TRANS)
    stages.append(gaps)
    return [g for g in stages if len(g) + 1 >= 96]


def test_every_gap_of_a_ridden_stage_can_hide_what_it_holds(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    from scream_amd import build as B
    src = os.path.join(REPO, "scream_amd", "csrc", "proj_ring.hip")
    out = tmp_path / "ring.s"
    subprocess.run(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", *B.SOURCES["proj_ring.hip"], "-S", "--cuda-device-only", "-o", str(out), src],
                   check=True, capture_output=True, timeout=600)
    m = re.search(r"^(\S*proj_ring_kernelINS_7SplitH2\S*):[^\n]*\n(.*?)\.Lfunc_end", out.read_text(), re.S | re.M)
    assert m, "proj_ring_kernel<SplitH2> not found"
    stages = _stages(m.group(2))
    ridden = [g for g in stages if sum(v for v, _ in g) >= 64]  # a ride: query 256, key ~350, value ~80 vector instructions in the gaps
    assert len(ridden) >= 6, "the ridden stages of the kernel were not found: %s" % [sum(v for v, _ in g) for g in stages]
    for g in ridden:
        assert max(t for _, t in g) <= 1, "a gap with %d transcendentals" % max(t for _, t in g)
        assert max(v for v, _ in g) <= 8, "a gap with %d vector instructions" % max(v for v, _ in g)
