"""x3 kernels beside their x6 twins: registers, spills (scratch) and LDS from hipcc's
-Rpass-analysis=kernel-resource-usage logs (the logs tools/kres.py reads).

usage: python3 tools/x3_kres.py LOG [LOG ...]      (exit status 1 if an x3 kernel uses scratch where
                                                    its x6 twin uses none)

A twin pair is two instantiations of one kernel template whose argument lists differ in exactly one
argument, 2 (x3's part count) against 3 (x6's)."""
import re
import shutil
import subprocess
import sys


def kernels(log):
    out, cur = {}, None
    for line in open(log, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def main():
    ks = {}
    for log in sys.argv[1:]:
        ks.update(kernels(log))
    names = sorted(ks)
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    by = {}
    for mangled, d in zip(names, dem):
        m = re.match(r"(?:void )?(?:spw::)?(\w+)<(.*)>\(", d)
        if m:
            by[(m.group(1), tuple(a.strip() for a in m.group(2).split(",")))] = ks[mangled]
    bad = 0
    f = lambda v, k: v.get(k, "?")
    print(f"{'kernel':58s} {'VGPR x6/x3':>11s} {'AGPR':>9s} {'spill':>9s} {'scratch B':>11s} {'occ':>5s} {'LDS':>15s}")
    for (name, args), v2 in sorted(by.items()):
        for i, a in enumerate(args):
            if a != "2":
                continue
            twin = by.get((name, args[:i] + ("3",) + args[i + 1:]))
            if twin is None:
                continue
            label = f"{name}<{','.join(args[:i] + ('NP',) + args[i + 1:])}>"
            sc3, sc2 = f(twin, "ScratchSize [bytes/lane]"), f(v2, "ScratchSize [bytes/lane]")
            print(f"{label[:58]:58s} {f(twin, 'VGPRs') + '/' + f(v2, 'VGPRs'):>11s} {f(twin, 'AGPRs') + '/' + f(v2, 'AGPRs'):>9s} "
                  f"{f(twin, 'VGPRs Spill') + '/' + f(v2, 'VGPRs Spill'):>9s} {sc3 + '/' + sc2:>11s} "
                  f"{f(twin, 'Occupancy [waves/SIMD]') + '/' + f(v2, 'Occupancy [waves/SIMD]'):>5s} "
                  f"{f(twin, 'LDS Size [bytes/block]') + '/' + f(v2, 'LDS Size [bytes/block]'):>15s}")
            if sc3 == "0" and sc2 != "0":
                bad += 1
                print("    ^ x3 uses scratch where x6 uses none")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
