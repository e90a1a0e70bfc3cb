"""Do two source trees compile to the same GPU code?  `python tools/isa_cmp.py OLD_CSRC NEW_CSRC [FILE.hip ...]`

Compiles every file of build.SOURCES (or only the files named) from both csrc directories to device assembly -- build.FLAGS plus
`--cuda-device-only -S`, from inside the directory so that no path reaches the output -- drops the lines that contain
`__hip_cuid_` (a symbol that is random per compilation, the only non-deterministic part) and compares the text.  One line per source
file: identical, or the names of the kernels / functions whose text differs; exit status 1 on any difference.  Each directory has to
sit in a whole tree (csrc includes ../../include/mi355asr.h): for the old one, e.g. `git archive PARENT | tar -x -C DIR`.
A refactor that moves helpers between files without touching what the kernels compute must leave every file identical."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tensorflowasr_amd import build as b  # noqa: E402


def device_asm(csrc, src):
    r = subprocess.run([b._hipcc()] + b.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: %s\n%s" % (csrc, src, r.stderr[-4000:]))
    return [ln for ln in r.stdout.splitlines() if "__hip_cuid_" not in ln]


def by_symbol(lines):
    """{symbol: text}: a function from its .type line to its .size line, a kernel descriptor with its kernel; the rest under ''"""
    out, cur = {"": []}, ""
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        out.setdefault(cur, []).append(ln)
        if cur and (re.match(r"\s*\.size\s+%s," % re.escape(cur), ln) or ".end_amdhsa_kernel" in ln):
            cur = ""
    return out


def compare(old, new, src):
    a, c = device_asm(old, src), device_asm(new, src)
    if a == c:
        return []
    sa, sc = by_symbol(a), by_symbol(c)
    return sorted(k or "(text outside the functions)" for k in set(sa) | set(sc) if sa.get(k) != sc.get(k))


def main():
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    srcs = sys.argv[3:] or b.SOURCES
    with ThreadPoolExecutor(max_workers=min(16, len(srcs))) as ex:
        diffs = list(ex.map(lambda s: compare(old, new, s), srcs))
    for s, d in zip(srcs, diffs):
        print("%-24s %s" % (s, "identical" if not d else "DIFFERENT: " + " ".join(d)), flush=True)
    return 1 if any(diffs) else 0


if __name__ == "__main__":
    sys.exit(main())
