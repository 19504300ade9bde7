"""Where the rides of csrc/proj_ring.hip stand in the generated code.  One wave per SIMD: behind a 32-cycle matrix instruction
about five 4-cycle vector instructions issue for free and at most one 8-cycle transcendental among them; what a gap holds beyond
that is paid in full while the neighbouring gaps hide nothing.  Two design rules follow, and both are properties of the code
hipcc makes, not of the source (left alone hipcc gathered a whole query chunk's elu + 1 behind ONE matrix instruction):

  * no gap between two matrix instructions of a stage holds more than one transcendental;
  * no gap holds more than eight vector instructions (8 x 4 cycles is the matrix instruction's own duration: a fuller gap
    cannot hide even in principle).

A stage is what stands between two s_barrier of proj_ring_kernel<SplitH2> with at least 96 matrix instructions."""
import re
import shutil

import pytest

TRANS = ("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")


def _stages(body):
    """per stage: the list of (vector instructions, transcendentals) of its gaps, in program order"""
    stages, gaps, v, t, seen = [], [], 0, 0, False
    for line in body:
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


def test_every_gap_of_a_ridden_stage_can_hide_what_it_holds():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    from scream_amd import asm_check, build
    found = [body for name, body in asm_check.kernels(build.assembly("proj_ring.hip")) if "proj_ring_kernelINS_7SplitH2" in name]
    assert found, "proj_ring_kernel<SplitH2> not found"
    stages = _stages(found[0])
    ridden = [g for g in stages if sum(v for v, _ in g) >= 64]  # a ride: query 256, key ~350, value ~80 vector instructions in the gaps
    assert len(ridden) >= 6, "the ridden stages of the kernel were not found: %s" % [sum(v for v, _ in g) for g in stages]
    for g in ridden:
        assert max(t for _, t in g) <= 1, "a gap with %d transcendentals" % max(t for _, t in g)
        assert max(v for v, _ in g) <= 8, "a gap with %d vector instructions" % max(v for v, _ in g)
