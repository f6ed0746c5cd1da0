"""Per-kernel register / spill / LDS / instruction-count report of a HIP source compiled for gfx950 (no GPU needed):
    python tools/kernel_regs.py understanding_flow_robustness_amd/csrc/igemm.hip [filter] [--text DIR]
`insts` = instructions of the kernel's body, `mfma` = the v_mfma_* among them.  --text DIR also writes, per kernel, the body with
comments, directives and label numbers stripped (DIR/<file>.<n>.<mangled name>.s): two builds whose files are equal emit the same
instruction stream.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

argv = sys.argv[1:]
text_dir = None
if "--text" in argv:
    i = argv.index("--text")
    text_dir = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
src = os.path.abspath(argv[0])
flt = argv[1] if len(argv) > 1 else ""
with tempfile.TemporaryDirectory() as d:
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
                    "-c", src, "-o", os.path.join(d, "x.o"), "-save-temps=obj"], check=True, stderr=subprocess.DEVNULL, cwd=d)
    s = open(next(os.path.join(d, f) for f in os.listdir(d) if f.endswith("gfx950.s"))).read()


def body(name):
    """The kernel's instructions: comments, directives, blank lines dropped; local labels renumbered in order of appearance."""
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M)
    lines, labels = [], {}
    for ln in m.group(1).split("\n"):
        ln = re.sub(r"\s*(;|//).*$", "", ln).strip()
        if not ln or (ln.startswith(".") and not ln.startswith(".L")):
            continue
        lines.append(ln)
    text = "\n".join(lines)
    for lab in re.findall(r"\.L[A-Za-z_]*\d+(?:_\d+)?", text):
        labels.setdefault(lab, f".L{len(labels)}")
    return re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", lambda mm: labels[mm.group(0)], text)


keys = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
for n, m in enumerate(re.finditer(r"- \.agpr_count:.*?\.wavefront_size", s, re.S)):
    meta = m.group(0)
    name = re.search(r"\.name:\s+(\S+)", meta).group(1)
    dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
    if flt and flt not in dn:
        continue
    num = lambda k: re.search(re.escape(k) + r":\s+(\d+)", meta).group(1)
    vals = " ".join(k[1:].replace("_count", "").replace("_fixed_size", "") + "=" + num(k) for k in keys)
    text = body(name)
    insts = [ln for ln in text.split("\n") if not ln.endswith(":")]
    vals += f" insts={len(insts)} mfma={sum(ln.startswith('v_mfma') for ln in insts)} text={hashlib.md5(text.encode()).hexdigest()[:8]}"
    if text_dir:
        os.makedirs(text_dir, exist_ok=True)
        with open(os.path.join(text_dir, f"{os.path.basename(src)}.{n:02d}.{name[:120]}.s"), "w") as f:
            f.write(text + "\n")
    print(dn[:80].ljust(80), vals)
