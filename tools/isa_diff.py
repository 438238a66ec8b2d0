#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 assembly two source trees compile to (CPU only: hipcc --cuda-device-only -S).
    python tools/isa_diff.py <tree A> <tree B> [source.hip ...]      # default: every entry of build.SOURCES
Every source is compiled in both trees with build.FLAGS + build.FILE_FLAGS of tree B.  Comment lines, trailing comments and the
.file / .ident / .loc / .section-style directives are dropped; every instruction line, the .amdhsa_* descriptor fields and the
kernel's metadata entry (registers, scratch, LDS, arguments) are kept.  A function is matched by its symbol across sources: one that moved is
compared in the source tree B has it in ("moved here") against wherever tree A had it.  Prints one markdown table row per source."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DROP = re.compile(r'\.(file|ident|loc|section|text|p2align|type|size|globl|protected|weak|hidden|addrsig\w*|cfi_\w+|amdgcn_target|amdhsa_code_object_version)\b')
LABEL = re.compile(r'\.L(BB|func_begin|func_end|tmp)\d+')


def functions(asm):
    """{symbol: normalised lines} of one assembly file: the body, the .amdhsa_kernel block and the metadata entry of each."""
    out, cur = {}, None
    for raw in asm.splitlines():
        start = re.match(r'([A-Za-z_$][\w$.]*):\s*; @', raw)
        line = raw.split(';')[0].rstrip()
        s = line.strip()
        if start:
            cur = out.setdefault(start.group(1), [])
        elif s.startswith('.amdhsa_kernel '):
            cur = out.setdefault(s.split()[1], [])
        elif re.match(r'  - \.\w+:', line):                  # one entry of amdhsa.kernels: its .name follows below
            cur = meta = []
        elif s.startswith('.name:') and cur is meta:
            cur = out.setdefault(s.split()[1], [])
            cur += meta
        elif raw.startswith('amdhsa.'):                      # a top-level metadata key: the file's last kernel entry ends here, not at the file's end
            cur = None
        if not s or DROP.match(s) or cur is None:
            continue
        cur.append(LABEL.sub(r'.L\1', s))
        if s.startswith(('.Lfunc_end', '.end_amdhsa_kernel', '.end_amdgpu_metadata')):
            cur = None
    return out


def assemble(tree, build, sources, tmp):
    def one(s):
        if not os.path.exists(os.path.join(tree, 'slotformer_amd', 'csrc', s)):
            return {}                                        # a source only the other tree has: every function of it differs
        dst = os.path.join(tmp, s + '.s')
        cmd = [build._hipcc()] + build.FLAGS + build.FILE_FLAGS.get(s, []) + (['-x', 'hip'] if s.endswith('.cpp') else []) + \
              ['--cuda-device-only', '-S', os.path.join(tree, 'slotformer_amd', 'csrc', s), '-o', dst]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(' '.join(cmd) + '\n' + r.stderr)
        with open(dst) as f:
            return functions(f.read())
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return dict(zip(sources, ex.map(one, sources)))


def main(a, b, *sources):
    spec = importlib.util.spec_from_file_location('sf_build', os.path.join(b, 'slotformer_amd', 'build.py'))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    sources = list(sources) or build.SOURCES
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, fb = assemble(a, build, sources, ta), assemble(b, build, sources, tb)
    # a function that moved between sources is matched by its symbol: compared where tree B has it, against wherever tree A had it
    home_a = {k: s for s in sources for k in fa[s]}
    home_b = {k: s for s in sources for k in fb[s]}
    print('| source | functions | instruction lines | moved here | differing |\n|---|---|---|---|---|')
    bad = 0
    for s in sources:
        moved = sorted(k for k in fb[s] if k not in fa[s] and k in home_a)
        gone = {k for k in fa[s] if k not in fb[s] and k in home_b}
        diff = sorted(k for k in (fa[s].keys() | fb[s].keys()) - gone if (fa[s] if k in fa[s] else fa[home_a.get(k, s)]).get(k) != fb[s].get(k))
        bad += len(diff)
        n = sum(1 for v in fb[s].values() for l in v if l[0].isalpha() and not l.endswith(':'))
        print(f"| {s} | {len(fb[s])} | {n} | {', '.join(f'{k} ({home_a[k]})' for k in moved) or 'none'} | {', '.join(diff) or 'none'} |")
    print(f'\n{bad} differing function(s) in {len(sources)} source(s)')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:]))
