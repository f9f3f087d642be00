"""Instruction counts per kernel of a translation unit's gfx950 ISA (hipcc -S --cuda-device-only): VALU / SALU / VMEM / LDS / total, VGPRs, SGPRs, scratch, LDS bytes,
flat loads and stores (an LDS or global access whose address space the compiler lost), the lane moves of SGPR spills (v_writelane + v_readlane), square roots (v_sqrt_*) and divisions (v_div_fixup_*).  Every instantiation of a kernel
template is listed under its own demangled name (k_shade<32u, 5>, k_trace<0, false, 2>, ...).
   python tools/isa_stats.py ti_raytrace_amd/csrc/tirt_trace.hip [kernel-name-substring ...]    (k_trace; tirt_render.hip for the shading kernels)
prints one line per kernel; used to show that a refactoring left the ISA alone."""
import hashlib, re, subprocess, sys, os, tempfile
src = sys.argv[1]; keys = sys.argv[2:]
d = os.path.dirname(os.path.abspath(src))
out = tempfile.mktemp(suffix=".s", dir="/tmp")
flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split() + os.environ.get("EXTRA", "").split()
subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.abspath(src)], cwd=d)
txt = open(out).read().split("\n"); os.unlink(out)
cur = None; body = False; stats = {}
for l in txt:
    m = re.match(r"^(_Z\w+):", l)
    if m: body = True; cur = m.group(1); stats[cur] = {"valu": 0, "salu": 0, "vmem": 0, "lds": 0, "total": 0, "hash": 0, "lane": 0, "sqrt": 0, "div": 0, "flat_ld": 0, "flat_st": 0}; continue
    if cur is None: continue
    t = l.strip()
    if t.startswith(".amdhsa_next_free_vgpr"): stats[cur]["vgpr_alloc"] = int(t.split()[1])
    if t.startswith(".amdhsa_group_segment_fixed_size"): stats[cur]["lds_bytes"] = int(t.split()[1])
    if t.startswith("; NumVgprs:"): stats[cur]["vgprs"] = int(t.split()[2])
    if t.startswith("; TotalNumSgprs:"): stats[cur]["sgprs"] = int(t.split()[2])
    if t.startswith("; ScratchSize:"): stats[cur]["scratch"] = int(t.split()[2])
    if t.startswith("; codeLenInByte"): stats[cur]["bytes"] = int(t.split()[-1])
    if t.startswith(".Lfunc_end"): body = False      # (what follows is the kernel's metadata, then other sections)
    if not body or not t or t[0] in ";." or t.endswith(":"): continue
    op = t.split()[0]
    s = stats[cur]; s["total"] += 1
    s["hash"] = (s["hash"] * 1000003 + int(hashlib.md5(re.sub(r"(\.Ltr_[a-z_]+?)\d+\b", r"\1", re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", t.split(";")[0]))).encode()).hexdigest()[:12], 16) ) & 0xffffffffffff      # (order-sensitive digest of the instruction text; the number an inline asm's %= puts into its .Ltr_* labels counts the asm blocks of the whole translation unit, not this kernel's: left out)
    if op.startswith(("v_writelane", "v_readlane")): s["lane"] += 1
    if op.startswith("flat_load_"): s["flat_ld"] += 1
    if op.startswith("flat_store_"): s["flat_st"] += 1
    if op.startswith("v_sqrt_"): s["sqrt"] += 1
    if op.startswith("v_div_fixup_"): s["div"] += 1
    if op.startswith("v_"): s["valu"] += 1
    elif op.startswith("s_"): s["salu"] += 1
    elif op.startswith("ds_"): s["lds"] += 1
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")): s["vmem"] += 1
import hashlib
for k, s in stats.items():
    if s["total"] == 0 or (keys and not any(x in k for x in keys)): continue
    dem = subprocess.run(["c++filt", k], stdout=subprocess.PIPE).stdout.decode().strip().split("(")[0].replace("void tirt::", "")
    print("%-44s VALU %5d SALU %5d VMEM %4d LDS %4d total %6d bytes %6s VGPRs %4s SGPRs %4s scratch %3s lane-moves %4d sqrt %3d div %3d LDS-bytes %5s flat-ld %2d flat-st %2d digest %012x"
          % (dem[:44], s["valu"], s["salu"], s["vmem"], s["lds"], s["total"], s.get("bytes"), s.get("vgprs"), s.get("sgprs"), s.get("scratch"), s["lane"], s["sqrt"], s["div"], s.get("lds_bytes"), s["flat_ld"], s["flat_st"], s["hash"]))
