"""Compare the device code of two builds kernel by kernel: instruction sequence, VGPRs, SGPRs, LDS, scratch.

usage: dp_kernel_identity.py BEFORE_DIR AFTER_DIR
Each directory holds what `hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -save-temps -Rpass-analysis=kernel-resource-usage
-c X.hip 2> X.resource.txt` left for its .hip files: the *-gfx950.s files and the remarks.  Every kernel of BEFORE must be in
AFTER with the same instructions (block labels renumbered: they carry the function's position in its file) and the same
resources.  Prints one line per kernel and ends with 1 if one is missing or differs."""
import glob
import os
import re
import sys


def kernels(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*gfx950.s"))):
        name, body = None, []
        for line in open(path):
            m = re.match(r"^(_Z\w+|k_\w+):", line)
            if m and name is None:
                name, body = m.group(1), []
                continue
            if name is not None:
                if line.startswith(".Lfunc_end"):
                    out[name] = body
                    name = None
                    continue
                s = line.split(";")[0].strip() if "s_waitcnt" not in line else line.strip()
                if s:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def resources(d):
    out, name = {}, None
    for path in sorted(glob.glob(os.path.join(d, "*resource.txt"))):
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {}
            m = re.search(r"remark: \S+ +(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def main():
    before, after = sys.argv[1], sys.argv[2]
    kb, ka, rb, ra = kernels(before), kernels(after), resources(before), resources(after)
    bad = 0
    print(f"{'kernel':72s} {'instr':>6s} {'SGPR':>5s} {'VGPR':>5s} {'AGPR':>5s} {'LDS':>6s} {'scratch':>7s}  verdict")
    for k in sorted(kb):
        r = rb.get(k, {})
        if k not in ka:
            verdict = "MISSING"
        elif kb[k] != ka[k]:
            verdict = "INSTRUCTIONS DIFFER"
        elif r != ra.get(k, {}):
            verdict = f"RESOURCES DIFFER {ra.get(k)}"
        else:
            verdict = "identical"
        bad += verdict != "identical"
        print(f"{k:72s} {len(kb[k]):6d} {r.get('TotalSGPRs', -1):5d} {r.get('VGPRs', -1):5d} {r.get('AGPRs', -1):5d} "
              f"{r.get('LDS', -1):6d} {r.get('ScratchSize', -1):7d}  {verdict}")
    extra = sorted(set(ka) - set(kb))
    print(f"{len(kb)} kernels before, {len(ka)} after, {bad} missing or different, new: {extra if extra else 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
