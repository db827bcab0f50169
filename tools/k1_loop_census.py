"""CPU: what the threshold kernel's row loop holds, per k_threshold instance, read from the compiler's assembly (which marks the blocks of a loop; a
disassembled code object does not): vector instructions, v_mov_b64 / v_mov_b32 among them, vector-memory instructions and the s_waitcnt vmcnt values in
program order -- inside the loop, and for the whole kernel with VGPRs, wavefronts per SIMD and scratch.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o k.s libcimbar_amd/csrc/cimbar_hip.hip && python tools/k1_loop_census.py k.s [name regex]
DESIGN.md section 3 (K1) has the table made with it."""
import collections, re, sys

pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
starts = lambda ops, p: sum(k for o, k in ops.items() if o.startswith(p))
for f in re.split(r"\n(?=_Z\w+:)", open(sys.argv[1]).read()):
    m = re.match(r"_ZN\d+(m\d+?)12_GLOBAL__N_111k_thresholdILi(\d)ELb(\d)ELi(\d+)E\w*:", f)
    if not m:
        continue
    name = f"{m.group(1)}::k_threshold<{m.group(2)}, {'true' if m.group(3) == '1' else 'false'}, {m.group(4)}>"
    if not pat.search(name):
        continue
    loop, whole, waits, inloop = collections.Counter(), collections.Counter(), [], False
    for l in f[:f.find(".Lfunc_end")].splitlines():
        if re.match(r"\.LBB\d+_\d+:", l) or l.startswith("; %bb."):
            inloop = "in Loop" in l or "Loop Header" in l
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            op = l.split()[0]
            whole[op] += 1
            if inloop:
                loop[op] += 1
                w = re.search(r"vmcnt\((\d+)\)", l) if op == "s_waitcnt" else None
                if w:
                    waits.append(w.group(1))
    g = lambda k: (re.search(r"; " + k + r": (\d+)", f) or [0, "?"])[1]
    print(f"{name}: loop: {starts(loop, 'v_')} vector instructions ({starts(loop, 'v_mov_b64')} v_mov_b64, {starts(loop, 'v_mov_b32')} v_mov_b32), "
          f"{starts(loop, 'global_') + starts(loop, 'buffer_')} vector-memory, vmcnt {' '.join(waits)} | kernel: {starts(whole, 'v_')} vector instructions, "
          f"{g('NumVgprs')} VGPRs, {g('Occupancy')} wavefronts per SIMD, scratch {g('ScratchSize')}")
