"""Compare two gfx950 code objects function by function: the proof that a refactor left the kernels alone.

    hipcc <the flags of build()> --offload-device-only --no-gpu-bundle-output -c -o a.elf eegnet_kernels.hip
    python tools/code_object_diff.py a.elf b.elf [substring-filter]

Per function: the instruction encodings (llvm-objdump's words, without addresses; branches are relative).
Per kernel: the 64-byte kernel descriptor from .rodata with its code-entry offset masked (it moves when an
earlier function changes size), and the whole metadata note (register counts, spills, LDS, arguments).
Prints one row per function that matches the filter, every function that differs, and ALL_IDENTICAL or
NOT_IDENTICAL.  The only other difference between two builds of unchanged kernels is the __hip_cuid_
symbol, a hash of the translation unit."""
import re
import subprocess
import sys

BIN = "/opt/rocm/llvm/bin/"


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def functions(elf):
    """symbol -> list of instruction encodings"""
    fs, cur = {}, None
    for line in run(BIN + "llvm-objdump", "-d", elf).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = fs.setdefault(m.group(1), [])
            continue
        m = re.search(r"//\s*[0-9A-Fa-f]+:\s*(.*)$", line)
        if cur is not None and m:
            cur.append(m.group(1).strip())
    return fs


def descriptors(elf):
    """kernel descriptor symbol -> its bytes, kernel_code_entry_byte_offset (bytes 16..23) zeroed"""
    ro = None
    for line in run(BIN + "llvm-readelf", "-S", "-W", elf).splitlines():
        m = re.search(r"\]\s+\.rodata\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            ro = (int(m.group(1), 16), int(m.group(2), 16))
    data = open(elf, "rb").read()
    out = {}
    for line in run(BIN + "llvm-readelf", "-s", "-W", elf).splitlines():
        p = line.split()
        if len(p) >= 8 and p[-1].endswith(".kd"):
            off = ro[1] + int(p[1], 16) - ro[0]
            kd = bytearray(data[off:off + int(p[2])])
            kd[16:24] = bytes(8)
            out[p[-1]] = bytes(kd)
    return out


def main():
    a, b = sys.argv[1], sys.argv[2]
    filt = sys.argv[3] if len(sys.argv) > 3 else "k_pass_e"
    fa, fb, ka, kb = functions(a), functions(b), descriptors(a), descriptors(b)
    names = sorted(set(fa) | set(fb))
    print(f"functions {len(fa)} vs {len(fb)}, kernel descriptors {len(ka)} vs {len(kb)}")
    for n in names:
        if filt in n:
            code = "identical" if fa.get(n) == fb.get(n) else "DIFFERENT"
            kd = "identical" if ka.get(n + ".kd") == kb.get(n + ".kd") else "DIFFERENT"
            print(f"  {n[:60]:60s} {len(fa.get(n, [])):6d} vs {len(fb.get(n, [])):6d} encodings: code {code}, descriptor {kd}")
    diff = [n for n in names if fa.get(n) != fb.get(n)]
    kdiff = [n for n in sorted(set(ka) | set(kb)) if ka.get(n) != kb.get(n)]
    for n in diff:
        print("  code differs:", n)
    for n in kdiff:
        print("  descriptor differs:", n)
    notes = run(BIN + "llvm-readelf", "--notes", a) == run(BIN + "llvm-readelf", "--notes", b)
    print(f"functions that differ {len(diff)}, descriptors that differ {len(kdiff)}, metadata note "
          f"{'identical' if notes else 'DIFFERENT'}")
    same = not diff and not kdiff and notes
    print("ALL_IDENTICAL" if same else "NOT_IDENTICAL")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
