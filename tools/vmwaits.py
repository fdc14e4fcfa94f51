"""Developer tool (no GPU): the `s_waitcnt vmcnt` waits hipcc put into the kernels of one csrc/*.hip file by itself, i.e. those
outside `;;#ASMSTART` .. `;;#ASMEND` (hand-written waits sit inside), per kernel with the basic block and the loop it lies in.
The file is compiled with build.py's flags plus `--cuda-device-only -S` into a temporary directory.
usage: python tools/vmwaits.py ss25_hierarchical_multiscale_image_classification_amd/csrc/conv_bf16.hip [kernel-name substring]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ss25_hierarchical_multiscale_image_classification_amd import build  # noqa: E402

WAIT = re.compile(r"^\s*s_waitcnt\b[^;]*\bvmcnt\((\d+)\)")
BLOCK = re.compile(r"^(\.LBB\d+_\d+):(.*)$")
LOOP = re.compile(r"(?:Loop Header|in Loop): (?:Header=)?(BB\d+_\d+)?\s*Depth=(\d+)")


def demangle(names):
    filt = shutil.which("llvm-cxxfilt")  # (binutils' c++filt misreads the __bf16 instantiations: mangled names are kept without it)
    if not filt or not names:
        return {n: n for n in names}
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def scan(asm_text):
    """[(kernel symbol, [(vmcnt, block label, loop description)])] for every .amdhsa_kernel of the listing"""
    lines = asm_text.split("\n")
    kernels = set(m.group(1) for m in (re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m)
    out, cur, waits, in_asm, block, loop = [], None, [], False, "entry", "-"
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in kernels:
            cur, waits, in_asm, block, loop = m.group(1), [], False, "entry", "-"
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", l):
            out.append((cur, waits))
            cur = None
            continue
        if "#ASMSTART" in l:
            in_asm = True
        elif "#ASMEND" in l:
            in_asm = False
        m = BLOCK.match(l)
        if m:
            block = m.group(1)
            # the loop comment is on the label's line ("=>This Loop Header: Depth=1", continued on the next lines) or on
            # the lines after it ("in Loop: Header=BB12_3 Depth=1")
            note = " ".join([m.group(2)] + [x for x in lines[i + 1:i + 4] if x.lstrip().startswith(";")])
            ml = LOOP.search(note)
            loop = "-" if not ml else f"loop {ml.group(1) or block[2:]} depth {ml.group(2)}"
        m = WAIT.match(l)
        if m and not in_asm:
            waits.append((int(m.group(1)), block, loop))
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    src, pick = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "out.s")
        subprocess.run([build._hipcc(), *build.FLAGS, "--cuda-device-only", "-S", src, "-o", asm], check=True)
        with open(asm) as f:
            found = scan(f.read())
    names = demangle([k for k, _ in found])
    for k, waits in found:
        if pick not in names[k]:
            continue
        print(f"{names[k]}: {len(waits)} compiler vmcnt wait(s)")
        for n, block, loop in waits:
            print(f"    vmcnt({n})  {block}  {loop}")


if __name__ == "__main__":
    main()
