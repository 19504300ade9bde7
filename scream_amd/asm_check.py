#!/usr/bin/env python3
"""Static check of hand-counted vector-memory waits in a hipcc-generated .s file.

The split GEMM and the layer-tail kernel load row operands with inline asm (`global_load_dwordx4 vN, ...`), so the
compiler does not know those registers are pending until a hand-placed `s_waitcnt vmcnt(N)`.  It may then legally copy,
spill or reuse such a register before the wait -- silently reading stale bytes.  This walks every kernel of the file in
program order with the in-order model of the vector-memory queue (loads, LDS-DMA and stores retire oldest first;
`vmcnt(N)` leaves the N youngest outstanding) and reports every instruction that touches a VGPR whose load is still
outstanding.  Second check (check_scalar_base_hazard): the wait states hipcc does not insert in front of an asm memory
instruction whose scalar base was just written by a VALU instruction.  Third and fourth: the data registers of a wide asm
store, and asm vector instructions that read a matrix-instruction result (check_store_data_hazard, check_mfma_asm_read_hazard).
gate() is what scream_amd/build.py refuses a library with: these four on every kernel, and no scratch for the kernels it names.

    python -m scream_amd.asm_check file.s [kernel-name-substring]
"""
import os
import re
import sys

REG = re.compile(r"\b([va])(\d+)\b|\b([va])\[(\d+):(\d+)\]")
ACC = 1000  # accumulation registers a0 .. a255 are tracked as 1000 .. 1255 (loads may target them on gfx90a and later)


def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(2)) + (ACC if m.group(1) == "a" else 0))
        else:
            base = ACC if m.group(3) == "a" else 0
            out.update(range(base + int(m.group(4)), base + int(m.group(5)) + 1))
    return out


def check_kernel(name, body, max_states_per_block=6):
    """body: list of asm lines of one kernel.  Walks the control-flow graph (every basic block with every distinct queue
    state that reaches it, capped per block) and returns a list of (line_no, text, registers) violations."""
    # ---- basic blocks
    label_at = {}
    for n, raw in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", raw)
        if m:
            label_at[m.group(1)] = n
    leaders = sorted(set([0] + list(label_at.values())))
    branch_re = re.compile(r"^\s*(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")
    for n, raw in enumerate(body):
        if branch_re.match(raw) or re.match(r"^\s*s_endpgm", raw):
            if n + 1 < len(body):
                leaders.append(n + 1)
    leaders = sorted(set(leaders))
    block_of = {}
    for k, st in enumerate(leaders):
        en = leaders[k + 1] if k + 1 < len(leaders) else len(body)
        block_of[st] = en

    def run_block(st, queue, bad):
        outstanding = [set(x) for x in queue]
        en = block_of[st]
        succ = [en] if en < len(body) else []
        for n in range(st, en):
            line = body[n].split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            op = line.split()[0]
            args = line[len(op):]
            mb = branch_re.match(body[n])
            if mb:
                tgt = label_at[mb.group(2)]
                succ = [tgt] if mb.group(1) == "s_branch" else [tgt] + ([en] if en < len(body) else [])
                continue
            if op == "s_endpgm":
                succ = []
                continue
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", line)
                if m:
                    keep = int(m.group(1))
                    outstanding = outstanding[len(outstanding) - keep:] if keep else []
                continue
            pending = set().union(*outstanding) if outstanding else set()
            is_vmem = op.startswith(("global_", "buffer_", "scratch_", "flat_"))
            touched = regs_of(args)
            if is_vmem and op.startswith("global_load") and "_lds_" not in op:
                dest = regs_of(args.split(",")[0])
                hit = ((touched - dest) & pending) | (dest & pending)
                if hit:
                    bad[n] = (n, line, sorted(hit))
                outstanding.append(dest)
            else:
                if touched & pending:
                    bad[n] = (n, line, sorted(touched & pending))
                if is_vmem:
                    outstanding.append(set())  # LDS-DMA, stores, scratch traffic: a queue slot, no VGPR result we track
            if len(outstanding) > 64:
                outstanding = outstanding[-64:]
        return succ, tuple(frozenset(x) for x in outstanding)

    bad = {}
    seen = {}
    work = [(0, ())]
    while work:
        st, queue = work.pop()
        states = seen.setdefault(st, set())
        if queue in states or len(states) >= max_states_per_block:
            continue
        states.add(queue)
        succ, out = run_block(st, queue, bad)
        for nx in succ:
            work.append((nx, out))
    return [bad[k] for k in sorted(bad)]


SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def sregs_of(text):
    out = set()
    for m in SREG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def check_scalar_base_hazard(name, body, need=5):
    """gfx9 / CDNA hazard: a VALU instruction that writes an SGPR (v_readlane_b32, v_readfirstlane_b32 -- how hipcc restores
    a spilled scalar -- or a VALU compare into an SGPR pair) must be `need` wait states away from a vector-memory instruction
    that reads that SGPR as its address.  hipcc pads its own memory instructions but does not look inside asm statements,
    which is where this project's register loads and stores with a scalar base live.  Straight-line scan backwards from every
    global_* instruction with an s[..] address (a label in between only shortens the distance seen: conservative)."""
    ins = []
    for raw in body:
        t = raw.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ins.append(t)
    bad = []
    for i, t in enumerate(ins):
        op = t.split()[0]
        if not op.startswith("global_") or " s[" not in t:
            continue
        addr = sregs_of(t.split(",")[-1])
        ws = 0
        for j in range(i - 1, -1, -1):
            tt = ins[j]
            o = tt.split()[0]
            if o.startswith("v_") and not o.startswith("v_mfma") and sregs_of(tt[len(o):].split(",")[0]) & addr:
                bad.append((i, t, tt, ws))
                break
            ws += int(tt.split()[1]) + 1 if o == "s_nop" else 1
            if ws >= need:
                break
    return bad


def check_store_data_hazard(name, body, need=2):
    """gfx9 / CDNA hazard: a vector-memory store of more than 64 bits reads its data VGPRs for a few cycles after issue; a
    VALU instruction that overwrites one of them within `need` wait states corrupts the stored value.  hipcc pads its own
    stores; an asm store is opaque to it."""
    ins = []
    for raw in body:
        t = raw.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ins.append(t)
    bad = []
    for i, t in enumerate(ins):
        if not re.match(r"global_store_dwordx[34]\b", t):
            continue
        data = regs_of(t.split(",")[1])
        ws = 0
        for j in range(i + 1, len(ins)):
            tt = ins[j]
            o = tt.split()[0]
            if o.startswith("v_") and regs_of(tt[len(o):].split(",")[0]) & data:
                bad.append((i, t, tt, ws))
                break
            ws += int(tt.split()[1]) + 1 if o == "s_nop" else 1
            if ws >= need:
                break
    return bad


ASM_VALU = re.compile(r"v_fma_mix(lo|hi)_f16\b|v_max_f32(_e32|_e64)? v\d+, 0, v\d+")  # the vector instructions the kernels write as inline asm


def check_mfma_asm_read_hazard(name, body, need=20):
    """A vector instruction that reads a VGPR written by a matrix instruction must be `need` wait states behind it (up to 18 for the
    16-pass ones; no hardware interlock).  hipcc pads the instructions it knows; GCNHazardRecognizer does not look inside inline asm.
    With accumulators in AGPRs a compiler-known v_accvgpr_read sits in between; proj_ring.hip is built with MFMA results in VGPRs
    and its rides read them through asm v_fma_mix.  Every intervening instruction counts as one wait state (a lower bound), in
    program order."""
    ins = []
    for raw in body:
        t = raw.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ins.append(t)
    last = {}  # VGPR -> (index, text) of the matrix instruction that wrote it last
    bad = []
    for i, t in enumerate(ins):
        o = t.split()[0]
        ops = t[len(o):].split(",")
        if o.startswith("v_mfma") or o.startswith("v_smfmac"):
            for r in regs_of(ops[0]):
                if r < ACC:
                    last[r] = i
            continue
        if ASM_VALU.match(t):
            for r in regs_of(",".join(ops[1:])):
                if r in last:
                    ws = sum((int(ins[k].split()[1]) + 1) if ins[k].startswith("s_nop") else 1 for k in range(last[r] + 1, i))
                    if ws < need:
                        bad.append((i, t, ins[last[r]], ws))
        if o.startswith(("v_", "ds_read", "ds_load", "global_load", "buffer_load")) and ops and ops[0].strip():
            for r in regs_of(ops[0]):
                last.pop(r, None)
    return bad


def kernels(path):
    lines = open(path).read().splitlines()
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    for k, (i, nm) in enumerate(starts):
        end = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), len(lines))
        yield nm, lines[i:end]




def private_segments(path):
    """kernel name -> .amdhsa_private_segment_fixed_size (bytes of scratch per lane) from the kernel descriptors of the file"""
    out, name = {}, None
    for l in open(path):
        w = l.split()
        if w[:1] == [".amdhsa_kernel"]:
            name = w[1]
        elif w[:1] == [".amdhsa_private_segment_fixed_size"]:
            out[name] = int(w[1])
    return out


def findings(name, body):
    """The check list: every violation of the four detectors in one kernel, one worded line each (gate() refuses with the first,
    main() prints them)."""
    out = ["touches a register whose asm load is still in flight: %s   <- pending %s" % (line, regs) for n, line, regs in check_kernel(name, body)]
    out += ["reads a matrix-instruction result with an asm vector instruction %d wait states behind it, fewer than 20 (%s ; %s)"
            % (ws, mf, t) for i, t, mf, ws in check_mfma_asm_read_hazard(name, body)]
    out += ["uses a scalar base %d wait states after a VALU write of it, fewer than 5 (%s -> %s)" % (ws, tt, t)
            for i, t, tt, ws in check_scalar_base_hazard(name, body)]
    out += ["overwrites the data of a wide store %d wait states behind it, fewer than 2 (%s ; %s)" % (ws, t, tt)
            for i, t, tt, ws in check_store_data_hazard(name, body)]
    return out


def gate(asm, asm_loads, no_scratch=(), want=""):
    """What a build must pass before it may run, on the assembly of the very object that will run (build.assembly).  asm_loads: the file
    requests operands with inline asm and waits for them with hand-counted s_waitcnt vmcnt(N) -- whether hipcc's register allocation
    respects that is a property of the generated code, so the four detectors run on every kernel whose mangled name contains `want`.
    no_scratch: name fragments; every kernel of the file whose name contains one must have a private segment of 0 bytes, and a fragment
    that matches no kernel is refused (a renamed kernel must not pass unseen).  Raises RuntimeError naming file, kernel and instruction;
    returns the number of kernels the detectors saw."""
    n = 0
    for name, body in kernels(asm) if asm_loads else ():
        if want not in name:
            continue
        n += 1
        bad = findings(name, body)
        if bad:
            raise RuntimeError("%s: %s %s (%d findings in this kernel; this hipcc allocates registers differently from the one the "
                               "kernels were written with)" % (asm, name, bad[0], len(bad)))
    sizes = private_segments(asm)
    for frag in no_scratch:
        named = [k for k in sizes if frag in k]
        if not named:
            raise RuntimeError("%s: no kernel named *%s* in the generated assembly" % (asm, frag))
        for k in named:
            if sizes[k]:
                raise RuntimeError("%s: %s uses %d bytes of scratch per lane (this hipcc allocates registers differently from the one "
                                   "the kernel was written with)" % (asm, k, sizes[k]))
    return n


def verify_source(src, flags, out_s, want=""):
    """Compile `src` to assembly with `flags` (the per-file flags of the object that will run) and put it through gate() with the
    build's table entry for that file; returns the number of kernels whose mangled name contains `want`.  For any build other than the
    one scream_amd/build.py verifies itself: whatever removes or adds memory operations changes what a hand-counted vmcnt(N) leaves
    in flight (round 2: a "no weight DMA" tuning variant of the layer tail -- since removed -- was launched with its ring waits
    still counting twelve pieces that no longer existed; the row operands were consumed while pending, their registers recycled
    as per-lane 64-bit addresses, the loads landed in them, and the next access left the aperture --
    HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION)."""
    from . import build
    asm_loads, no_scratch = build.GATE.get(os.path.basename(src), (True, ()))
    return gate(build.assembly(src, flags, out_s), asm_loads, no_scratch, want)


def main():
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    total = 0
    for nm, body in kernels(sys.argv[1]):
        if want not in nm:
            continue
        bad = findings(nm, body)
        n_asm = sum(1 for l in body if re.match(r"\s*global_load_dwordx4 [va]", l))
        print("%s: %d register loads, %d violations" % (nm[:70], n_asm, len(bad)))
        for text in bad[:12]:
            print("   " + text)
        total += len(bad)
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
