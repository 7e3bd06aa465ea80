"""Static instruction report of the device code, CPU only: compiles a .hip file device-side to gfx950 assembly with the
Makefile's HIPFLAGS and counts, per kernel and per basic block, the instruction kinds that round 5 was about:
  valu     every v_* instruction (lane moves included: they issue on the vector ALU)
  salu     s_* arithmetic / moves / compares (no branches, waits, barriers, scalar loads)
  copies   v_mov_b32 vA, vB -- a plain VGPR-to-VGPR copy, what a failed register coalescing leaves behind
  lane     v_readlane / v_writelane (SGPR spills to lanes of a VGPR and their reloads)
  scratch  scratch_* loads and stores (VGPR spills)
plus the register and spill counts of the kernel's metadata.  It counts nothing else.  listing() keeps every block's
instructions and the compiler's loop notes, for questions the report does not ask (tests/test_shade_isa_cpu.py).
usage: python scripts/isa_report.py [file.hip ...] [--filter SUBSTR] [--min-valu 8] [--no-blocks] [--asm-out DIR]
       (default file: path_tracing_amd/csrc/pt_trace.hip)
       python scripts/isa_report.py --digest [file.hip ...]    one line per kernel: name, instructions, SHA-256 of its body
       (comments left out, the function number taken out of local labels) -- two trees whose listings agree run the same device code"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
KINDS = ("valu", "salu", "copies", "lane", "scratch")
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")

_NOT_SALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_sleep", "s_setprio", "s_sendmsg",
             "s_trap", "s_code_end", "s_load", "s_buffer_load", "s_icache", "s_inst_prefetch", "s_sethalt", "s_setkill")
_COPY = re.compile(r"^v_mov_b32(_e32)?\s+v\d+,\s*v\d+\s*$")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_FALLTHROUGH = re.compile(r"^;\s*%bb\.(\d+):")
_DEPTH_OWN = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
_DEPTH_IN = re.compile(r"in Loop: Header=\S+ Depth=(\d+)")


def find_hipcc():
    """Path of hipcc, or None."""
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def makefile_hipflags(makefile=None):
    """The HIPFLAGS of csrc/Makefile as a list, $(ARCH) expanded with the Makefile's default."""
    text = open(makefile or os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_asm(src, extra=(), out=None):
    """Device-only assembly of `src` (a .hip file) with the Makefile's flags; returns the text."""
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    src, tmp = os.path.abspath(src), None
    if out is None:
        tmp = tempfile.mkdtemp(prefix="isa_report_")
        out = os.path.join(tmp, os.path.basename(src) + ".s")
    try:
        subprocess.check_call([hipcc] + makefile_hipflags() + list(extra) + ["--cuda-device-only", "-S", "-o", out, src],
                              cwd=os.path.dirname(os.path.abspath(src)))
        return open(out).read()
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


def classify(line):
    """The kinds (a subset of KINDS) that one assembly line counts towards."""
    code = line.split(";", 1)[0].strip()
    if not code or code[0] == "." or code.endswith(":"):
        return ()
    op = code.split(None, 1)[0]
    if op.startswith("v_"):
        if op.startswith("v_readlane") or op.startswith("v_writelane"):
            return ("valu", "lane")
        if _COPY.match(code):
            return ("valu", "copies")
        return ("valu",)
    if op.startswith("s_"):
        return () if op.startswith(_NOT_SALU) else ("salu",)
    if op.startswith("scratch_"):
        return ("scratch",)
    return ()


def _metadata(asm):
    """{kernel symbol: {register / spill counts}} from the amdhsa.kernels notes."""
    out, cur = {}, None
    inside = False
    for line in asm.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line.startswith("amdhsa.") or line.startswith("..."):
            break
        if line.startswith("  - "):
            cur = {}
            out[id(cur)] = cur
        m = re.match(r"^  (?:- |  )\.(\w+):\s*(.*)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip()
    named = {}
    for d in out.values():
        if "name" in d:
            named[d["name"].strip("'\"")] = {k: int(d[k]) for k in META_KEYS if k in d}
    return named


def short_name(symbol):
    """k_trace<0,0,1,0> for _Z7k_traceILb0ELb0ELb1ELb0EEv...; other symbols demangled without their parameter list
    where a demangler is at hand, else unchanged."""
    m = re.match(r"^_ZN?", symbol)
    if not m:
        return symbol
    pos, name = m.end(), None
    while True:                                               # length-prefixed components; the last one is the function
        d = re.match(r"\d+", symbol[pos:])
        if not d:
            break
        n = int(d.group(0)); pos += d.end()
        name = symbol[pos:pos + n]; pos += n
    if name is None:
        return symbol
    t = re.match(r"I((?:Lb[01]E)+)E", symbol[pos:])
    return "%s<%s>" % (name, ",".join(re.findall(r"Lb([01])E", t.group(1)))) if t else name


def parse(asm):
    """[{symbol, name, counts{kind: n}, meta{...}, blocks[{label, depth, counts}]}] for every kernel of an assembly text
    (a kernel = a function that the metadata lists)."""
    meta = _metadata(asm)
    kernels, cur, block = [], None, None
    lines = asm.splitlines()
    for i, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in meta:
            cur = {"symbol": m.group(1), "name": short_name(m.group(1)), "counts": dict.fromkeys(KINDS, 0),
                   "meta": meta[m.group(1)], "blocks": []}
            block = {"label": "entry", "depth": 0, "counts": dict.fromkeys(KINDS, 0)}
            cur["blocks"].append(block)
            kernels.append(cur)
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = block = None
            continue
        s = line.strip()
        lab = _LABEL.match(s)
        ft = _FALLTHROUGH.match(s) if not lab else None
        if lab or ft:
            # the loop annotation is on the label's line and the comment lines right after it
            note = s
            j = i + 1
            while j < len(lines) and lines[j].strip().startswith(";"):
                note += " " + lines[j]
                j += 1
            d = _DEPTH_OWN.search(note) or _DEPTH_IN.search(note)
            if ft and ft.group(1) == "0":
                continue                                      # the entry block's own comment
            block = {"label": lab.group(1) if lab else "%bb." + ft.group(1), "depth": int(d.group(1)) if d else 0,
                     "counts": dict.fromkeys(KINDS, 0)}
            cur["blocks"].append(block)
            continue
        for k in classify(line):
            cur["counts"][k] += 1
            block["counts"][k] += 1
    return kernels


_ZERO_MOVE = re.compile(r"^v_mov_b32(_e32)?\s+v\d+,\s*0\s*$")


def listing(asm):
    """{kernel name: [{label, note, code[...]}]}: every basic block of every kernel with its instructions (comments cut) and
    the compiler's loop note (the label's line and the comment lines after it)."""
    meta = _metadata(asm)
    out, cur, block = {}, None, None
    lines = asm.splitlines()
    for i, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in meta:
            block = {"label": "entry", "note": "", "code": []}
            cur = out.setdefault(short_name(m.group(1)), [])
            cur.append(block)
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = block = None
            continue
        s = line.strip()
        lab = _LABEL.match(s)
        ft = _FALLTHROUGH.match(s) if not lab else None
        if lab or ft:
            note, j = s, i + 1
            while j < len(lines) and lines[j].strip().startswith(";"):
                note += " " + lines[j].strip()
                j += 1
            if ft and ft.group(1) == "0":
                continue
            block = {"label": lab.group(1) if lab else "%bb." + ft.group(1), "note": note, "code": []}
            cur.append(block)
            continue
        code = line.split(";", 1)[0].strip()
        if code and code[0] != "." and not code.endswith(":"):
            block["code"].append(code)
    return out


_LOCAL_LABEL = re.compile(r"(\.LBB|\.Lfunc_[A-Za-z_]*)\d+")


def digests(asm):
    """[(name, instructions, sha256 of the body)] for every kernel of an assembly text.  The body is every line of code
    (instructions, labels, directives) from the kernel's label to its .Lfunc_end.  The function's number in local labels
    is dropped (.LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end), which is all that moving a kernel inside a file or to
    another file changes in the code; the compiler's comments are left out, because its loop notes repeat those numbers
    and are padded to a column by the label's length.  Nothing else is altered."""
    meta = _metadata(asm)
    out, cur = [], None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in meta:
            cur = [short_name(m.group(1)), 0, hashlib.sha256()]
            out.append(cur)
        elif cur is not None and line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            code = line.split(";", 1)[0].strip()
            if code:
                cur[1] += code[0] != "." and not code.endswith(":")
                cur[2].update((_LOCAL_LABEL.sub(r"\1", code) + "\n").encode())
    return [(name, n, h.hexdigest()) for name, n, h in out]


def report(src, extra=()):
    """parse(compile_asm(src))"""
    return parse(compile_asm(src, extra))


def format_kernels(kernels):
    rows = ["| kernel | VALU | SALU | copies | lane | scratch | VGPRs | SGPRs | VGPR spills | SGPR spills |", "|---|---|---|---|---|---|---|---|---|---|"]
    for k in kernels:
        c, m = k["counts"], k["meta"]
        rows.append("| `%s` | %d | %d | %d | %d | %d | %s | %s | %s | %s |" % (
            k["name"], c["valu"], c["salu"], c["copies"], c["lane"], c["scratch"], m.get("vgpr_count", "?"),
            m.get("sgpr_count", "?"), m.get("vgpr_spill_count", "?"), m.get("sgpr_spill_count", "?")))
    return "\n".join(rows)


def format_blocks(kernel, min_valu=8):
    rows = ["`%s`, blocks of %d or more VALU:" % (kernel["name"], min_valu), "",
            "| block | loop depth | VALU | SALU | copies | lane | scratch |", "|---|---|---|---|---|---|---|"]
    for b in kernel["blocks"]:
        c = b["counts"]
        if c["valu"] >= min_valu:
            rows.append("| %s | %d | %d | %d | %d | %d | %d |" % (b["label"], b["depth"], c["valu"], c["salu"], c["copies"], c["lane"], c["scratch"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", default=[os.path.join(CSRC, "pt_trace.hip")])
    ap.add_argument("--filter", default="", help="only kernels whose name contains this")
    ap.add_argument("--min-valu", type=int, default=8)
    ap.add_argument("--no-blocks", action="store_true")
    ap.add_argument("--asm-out", default=None, help="keep the assembly in this directory")
    ap.add_argument("--from-asm", action="store_true", help="the files are assembly already")
    ap.add_argument("--digest", action="store_true", help="per kernel: name, instruction count, SHA-256 of the body (see digests)")
    a = ap.parse_args()
    if a.digest:
        for f in a.files:
            for name, n, h in sorted(digests(open(f).read() if a.from_asm else compile_asm(f))):
                if a.filter in name:
                    print("%-44s %6d  %s" % (name, n, h))
        return
    for f in a.files:
        if a.from_asm:
            asm = open(f).read()
        else:
            out = None
            if a.asm_out:
                os.makedirs(a.asm_out, exist_ok=True)
                out = os.path.join(os.path.abspath(a.asm_out), os.path.basename(f) + ".s")
            asm = compile_asm(f, out=out)
        ks = [k for k in parse(asm) if a.filter in k["name"] or a.filter in k["symbol"]]
        print("## %s\n" % os.path.relpath(f, ROOT) if not a.from_asm else "## %s\n" % f)
        print(format_kernels(ks))
        if not a.no_blocks:
            for k in ks:
                print()
                print(format_blocks(k, a.min_valu))
        print()


if __name__ == "__main__":
    main()
