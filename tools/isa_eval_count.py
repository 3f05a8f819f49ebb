"""Static instruction counts of ONE patch evaluation (hypothesis x source view) in the timed kernels, from the gfx950 assembly the product is built from: per kernel, every
loop (label .. backward branch) that contains the tap rows' `buffer_load_dwordx4 ... idxen`, innermost first, with its instructions by class.  In pm_sweep2_kernel the loop
of ~1 550 (photometric) / ~1 780 (geometric) instructions is pm_visit's loop over the lane's views, i.e. one evaluation with its rare paths; in the speculative kernels
the smallest loop around the tap rows is a whole trip.  No GPU needed:
    python tools/isa_eval_count.py [-DPM_PROBE_... ...]          (profiles/eval_trim_isa_counts.txt)"""
import collections, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix as im

KERNELS = ("pm_sweep2_kernelILi4ELi2ELb0ELb1ELb0", "pm_sweep2_kernelILi4ELi2ELb1ELb1ELb0", "pm_sweep_widen_kernelILb0ELi2ELb1ELb0", "pm_sweep_widen_kernelILb1ELi2ELb1ELb0",
           "pm_init_kernelILi4ELb0ELi2ELi4", "pm_init_kernelILi4ELb1ELi2ELi4")


def loops(body):
    labels, out = {}, []
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and m.group(1) in labels:
            out.append((labels[m.group(1)], i))
    return out


def mix(seg):
    c = collections.Counter()
    for ln in seg:
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        c[im.classify(s.split()[0])] += 1
    return c


def valu(c):
    return c["valu"] + c["valu_packed"] + c["valu_cmp"] + c["valu_trans"] + c["valu_lane"]


if __name__ == "__main__":
    im._b.FLAGS = im._b.FLAGS + [a for a in sys.argv[1:] if a.startswith("-D")]
    for name, body in im.kernels(im.assembly()):
        if not any(k in name for k in KERNELS):
            continue
        tot = mix(body)
        print("%s: %d instructions, VALU %d (lane moves %d), LDS %d, SALU %d, scratch %d" % (im.demangle(name), sum(tot.values()), valu(tot), tot["valu_lane"], tot["lds"], tot["salu"],
                                                                                              sum(1 for l in body if "scratch_" in l)))
        for a, b in sorted([(a, b) for a, b in loops(body) if any("idxen" in l for l in body[a:b])], key=lambda x: x[1] - x[0]):
            c = mix(body[a:b + 1])
            print("    loop of %5d instructions: VALU %5d (lane moves %d), LDS %d, vector memory %d, SALU %d" % (sum(c.values()), valu(c), c["valu_lane"], c["lds"], c["vmem"], c["salu"]))
