"""Where the stage loop of k_split_reg<N, NR> waits for memory, read off the compiled listing (profiles/stage_waits.md):

  python tools/stage_waits.py [N [NR]] [--asm FILE] [-DSPLITR_...=..]

  * the warm-up of the next stage's coefficient record (SPLITR_KWARM): the single-dword loads of the loop, and how many vector
    instructions lie between the last of them and the first following s_waitcnt that names lgkmcnt;
  * the reads of the uniform factor G(r) (the 2^NR ds_read_b128 on one address register with offsets 16 k): for each, the fp64
    instructions between the read and the s_waitcnt that releases its value (LDS results return in order: the first wait whose
    count is not larger than the number of LDS / scalar-memory instructions issued since);
  * the same for the table reads of expmi (the other ds_read_b128 in front of the first G read);
  * the counts that must not move: fp64, DPP moves, swaps, barriers, scratch, vector registers.

--asm FILE reads a listing made earlier (hipcc -S --cuda-device-only of rydemu_splitreg.hip) instead of compiling."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGKM = re.compile(r"^\s+(ds_|s_load_|s_buffer_load_)")


def listing(n, defs):
    src = os.path.join(ROOT, "pulser_amd", "csrc", "rydemu_splitreg.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "r.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Wno-unused-value", "-Wno-unused-function", f"-DRYD_SPLITR_N={n}", *defs, src,
                        "-o", asm], check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def stage_loop(text, n, nr):
    """(lines of the longest depth-1 loop of k_split_reg<n, nr, plain>, its vector register count)"""
    name = r"_Z\d+k_split_regILi%dELi%dELb0ELb0ELb0ELb0E\w*" % (n, nr)
    m = re.search(r"^(%s):(.*?)s_endpgm" % name, text, re.S | re.M)
    body = m.group(2).split("\n")
    best = None
    for hdr in [i for i, l in enumerate(body) if "Loop Header: Depth=1" in l]:
        lab = body[hdr].split(":")[0]
        backs = [i for i, l in enumerate(body) if re.search(r"s_c?branch\w*\s+%s\b" % re.escape(lab), l)]
        if backs and (best is None or backs[-1] - hdr > best[1] - best[0]):
            best = (hdr, backs[-1])
    meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % name, text, re.S).group(1)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    return body[best[0]:best[1] + 1], vgpr


def release(reg, i):
    """index of the s_waitcnt that releases the LDS read at line i, or None"""
    issued = 0
    for j in range(i + 1, len(reg)):
        if LGKM.search(reg[j]):
            issued += 1
            continue
        w = re.search(r"s_waitcnt.*lgkmcnt\((\d+)\)", reg[j])
        if w and int(w.group(1)) <= issued:
            return j
    return None


def analyse(reg, nr):
    na = 1 << nr
    c = lambda pat, lines=reg: sum(1 for l in lines if re.search(pat, l))
    fp64 = lambda a, b: c(r"^\s+v_\w+_f64", reg[a:b])
    out = {"fma": c(r"\sv_fmac?_f64"), "mul": c(r"\sv_mul_f64"), "add": c(r"\sv_add_f64"), "rndne": c(r"v_rndne_f64"),
           "dpp": c(r"v_mov_b32_dpp"), "swap": c(r"v_permlane\d+_swap"), "barriers": c(r"s_barrier"), "scratch": c(r"scratch_")}
    # the warm-up: single-dword scalar loads (every other scalar load of the stage is wider) or the one vector load
    warm = [i for i, l in enumerate(reg) if re.search(r"^\s+(s_load_dword|global_load_dword)\s", l)]
    out["warm_loads"] = len(warm)
    out["warm_kind"] = "-" if not warm else reg[warm[-1]].split()[0]
    if warm:
        nxt = next((j for j in range(warm[-1] + 1, len(reg)) if re.search(r"s_waitcnt.*lgkmcnt", reg[j])), len(reg))
        out["warm_valu_to_wait"] = c(r"^\s+v_", reg[warm[-1] + 1:nxt])
    else:
        out["warm_valu_to_wait"] = 0
    # the G table: the address register with 2^NR ds_read_b128 at the offsets 16 k
    reads = {}
    for i, l in enumerate(reg):
        m = re.match(r"\s+ds_read_b128 v\[\d+:\d+\], (v\d+)(?: offset:(\d+))?\s*$", l)
        if m:
            reads.setdefault(m.group(1), []).append((i, int(m.group(2) or 0)))
    # (the table's own LDS offset may ride in the instruction: offsets base + 16 k)
    gbase = {r: min(o for _, o in v) for r, v in reads.items()}
    gregs = [r for r, v in reads.items() if sorted(o - gbase[r] for _, o in v) == [16 * k for k in range(na)]]
    assert len(gregs) == 1, f"G table reads not found: {dict((r, len(v)) for r, v in reads.items())}"
    dist = []
    for i, off in reads[gregs[0]]:
        j = release(reg, i)
        dist.append(((off - gbase[gregs[0]]) // 16, fp64(i, j) if j is not None else -1))
    out["g_reads"] = dist
    first_g = min(i for i, _ in reads[gregs[0]])
    tdist = []
    for r, v in reads.items():
        if r == gregs[0]:
            continue
        for i, _ in v:
            if i < first_g:
                j = release(reg, i)
                tdist.append(fp64(i, j) if j is not None else -1)
    out["trig_reads"] = tdist
    return out


def main(argv):
    defs = [a for a in argv if a.startswith("-D")]
    pos = [a for a in argv if not a.startswith("-")]
    asm = None
    if "--asm" in argv:
        asm = argv[argv.index("--asm") + 1]
        pos = [a for a in pos if a != asm]
    n = int(pos[0]) if pos else 14
    nr = int(pos[1]) if len(pos) > 1 else 5
    text = open(asm).read() if asm else listing(n, defs)
    reg, vgpr = stage_loop(text, n, nr)
    r = analyse(reg, nr)
    g = [d for _, d in r["g_reads"]]
    print(f"# waits of the stage loop of `k_split_reg<{n}, {nr}>` ({' '.join(defs) or 'default switches'})\n")
    print("| warm-up loads | kind | VALU from the last one to the next lgkmcnt wait | G reads | fp64 between a G read and its wait: min | median | max "
          "| table reads of expmi | fp64 to their wait: min | fma | mul | add | rndne | v_mov_b32_dpp | v_permlane*_swap | barriers | scratch | vector registers |")
    print("|" + "---|" * 18)
    print(f"| {r['warm_loads']} | {r['warm_kind']} | {r['warm_valu_to_wait']} | {len(g)} | {min(g)} | {sorted(g)[len(g) // 2]} | {max(g)} "
          f"| {len(r['trig_reads'])} | {min(r['trig_reads']) if r['trig_reads'] else '-'} | {r['fma']} | {r['mul']} | {r['add']} | {r['rndne']} "
          f"| {r['dpp']} | {r['swap']} | {r['barriers']} | {r['scratch']} | {vgpr} |")
    print("\nG(r) by register r: " + " ".join(f"{k}:{d}" for k, d in sorted(r["g_reads"])))


if __name__ == "__main__":
    main(sys.argv[1:])
