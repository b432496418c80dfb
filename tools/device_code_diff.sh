#!/bin/bash
# device code of every csrc/*.hip, working tree against a git revision: tools/device_code_diff.sh <rev> [file.hip ...]
# Both sides are compiled device-only with the build's own flags (build.py: FLAGS + PER_FILE_FLAGS) and the .text and .rodata sections
# of the two gfx950 code objects are compared byte for byte.  Where the sections differ (a host-side edit can change the order in which
# templates are instantiated, which moves functions within .text) every function symbol is compared instead: name, size and bytes.
# Exit status 0: every file identical (by section or by symbol).  A host-only refactor is proven neutral for the kernels here, not on a GPU.
REV=${1:-HEAD}; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LLVM=${LLVM_BIN:-/opt/rocm/llvm/bin}
W=$(mktemp -d /tmp/sslcr_devdiff.XXXXXX); trap 'rm -rf $W' EXIT
mkdir -p $W/old/ssl_cr_histo_amd/csrc $W/old/include $W/new/ssl_cr_histo_amd/csrc $W/new/include
FILES=${@:-$(cd $ROOT/ssl_cr_histo_amd/csrc && ls *.hip)}
cp $ROOT/ssl_cr_histo_amd/csrc/*.hpp $W/new/ssl_cr_histo_amd/csrc/; cp $ROOT/include/sslcr.h $W/new/include/
for f in $(git -C $ROOT ls-tree --name-only $REV ssl_cr_histo_amd/csrc/ | grep '\.hpp$'); do git -C $ROOT show $REV:$f > $W/old/$f; done
git -C $ROOT show $REV:include/sslcr.h > $W/old/include/sslcr.h
status=0
for f in $FILES; do
  git -C $ROOT show $REV:ssl_cr_histo_amd/csrc/$f > $W/old/ssl_cr_histo_amd/csrc/$f 2>/dev/null || { echo "### $f: not in $REV"; continue; }
  cp $ROOT/ssl_cr_histo_amd/csrc/$f $W/new/ssl_cr_histo_amd/csrc/
  flags=$(cd $ROOT/ssl_cr_histo_amd && python3 -c "import build, sys; print(' '.join(build.FLAGS + build.PER_FILE_FLAGS.get(sys.argv[1], [])))" $f)
  for side in old new; do
    ( /opt/rocm/bin/hipcc $flags --cuda-device-only --no-gpu-bundle-output -x hip -c $W/$side/ssl_cr_histo_amd/csrc/$f -o $W/$side.co 2> $W/$side.err &&
      for sec in text rodata; do $LLVM/llvm-objcopy -O binary --only-section=.$sec $W/$side.co $W/$side.$sec; done &&
      $LLVM/llvm-readelf -S -s --wide $W/$side.co > $W/$side.sym ) &
  done; wait
  if [ ! -s $W/old.sym ] || [ ! -s $W/new.sym ]; then echo "### $f: COMPILE FAILED"; cat $W/old.err $W/new.err | head -20; status=1; continue; fi
  python3 - "$f" $W <<'PY' || status=1
import re, sys
f, w = sys.argv[1], sys.argv[2]
rd = lambda side, ext: open(f"{w}/{side}.{ext}", "rb").read()
size = {s: len(rd("new", s)) for s in ("text", "rodata")}
if all(rd("old", s) == rd("new", s) for s in ("text", "rodata")):
    print(f"### {f}: identical  (.text {size['text']} B, .rodata {size['rodata']} B, byte for byte)")
    sys.exit(0)
def symbols(side):
    """function name -> bytes; .rodata object name -> bytes.  A kernel descriptor (<kernel>.kd, 64 bytes) holds the distance to its
    kernel's entry at bytes 16..23: that field is checked to point at the kernel of the same name and left out of the bytes"""
    sym, sec = rd(side, "sym").decode(), {s: rd(side, s) for s in ("text", "rodata")}
    base = {s: int(re.search(r"\]\s+\." + s + r"\s+PROGBITS\s+([0-9a-f]+)", sym).group(1), 16) for s in sec}
    rows = [(m.group(3), m.group(4), int(m.group(1), 16), int(m.group(2)))
            for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+\d+\s+(\S+)", sym, re.M)]
    addr = {name: v for kind, name, v, n in rows if kind == "FUNC"}
    d = {}
    for kind, name, v, n in rows:
        s = "text" if kind == "FUNC" else "rodata"
        if not base[s] <= v < base[s] + len(sec[s]): continue             # (an object of another section)
        data = sec[s][v - base[s]:v - base[s] + n]
        if kind == "OBJECT" and name.endswith(".kd") and n == 64:
            entry = v + int.from_bytes(data[16:24], "little", signed=True)
            data = data[:16] + data[24:] + (b"entry ok" if addr.get(name[:-3]) == entry else b"entry elsewhere %d" % entry)
        d[kind + " " + name] = data
    return d
a, b = symbols("old"), symbols("new")
bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
nf, nk = sum(k.startswith("FUNC") for k in b), sum(k.endswith(".kd") for k in b)
if not bad:
    old_size = {s: len(rd("old", s)) for s in size}
    pad = "" if size == old_size else f"; padding between them: .text {old_size['text']} -> {size['text']} B"
    print(f"### {f}: identical per symbol  ({nf} functions and {nk} kernel descriptors: name, size and bytes; their ORDER within "
          f".text / .rodata differs, i.e. the order in which the host code instantiates the templates{pad})")
    sys.exit(0)
print(f"### {f}: DIFFERS  ({len(bad)} of {len(b)} symbols)")
for k in bad[:20]: print("   ", k[-100:], len(a.get(k, b"")), "->", len(b.get(k, b"")))
sys.exit(1)
PY
done
[ $status = 0 ] && echo "device code unchanged against $REV" || echo "DEVICE CODE CHANGED against $REV"
exit $status
