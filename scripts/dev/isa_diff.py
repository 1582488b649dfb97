#!/usr/bin/env python3
"""Developer tool: compare the gfx950 code objects of two revisions function by function.

    # device code object of sr_fit.hip at any revision (the flags of spinrelax_amd/build.py, device only):
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -ffp-contract=off --offload-device-only \
        -c spinrelax_amd/csrc/sr_fit.hip -o a.co
    # where hipcc wraps the code object in an offload bundle (llvm-objdump: "not recognized as a valid object file"):
    /opt/rocm/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=a.co --output=a.elf
    scripts/dev/isa_diff.py a.elf b.elf 'k_trf|k_order_search|search_order'      # or a.co b.co where they are plain code objects
    # a side may be several code objects, joined with commas: code that moved between sources, e.g. the parent's sr_ct.hip
    # against the files it was split into (add -fno-slp-vectorize, as build.py does for them)
    scripts/dev/isa_diff.py old/sr_ct.elf sr_pack.elf,sr_ct.elf,sr_ct_direct.elf,sr_ct_fft64.elf,sr_ct_rfft64.elf

Disassembles them with llvm-objdump -d, cuts the listing at every function symbol, drops addresses and encodings, writes branch
targets as symbol + offset instead of a word offset and masks the offsets of pc-relative addresses (a function that only moved
inside the object is not a change) and prints, per function whose demangled name matches the pattern, "same" or the number of
differing instruction lines; functions present on only one side are listed as such.  The function maps of one side's objects
are merged; a name that two of them define is an error (which of the two would be compared?).  Exit status 1 if any differ."""
import re
import subprocess
import sys

OBJDUMP = '/opt/rocm/llvm/bin/llvm-objdump'


def functions(co):
    txt = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', '--no-leading-addr', '-C', co], capture_output=True, text=True,
                         check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        code, _, comment = line.partition('//')
        ins = re.sub(r'<[^>]*>', '<>', code.strip())
        if not ins or ins == '...':        # '...': objdump's mark for the zero padding behind the last function of the section -- it
            continue                       # moves to another function when the functions change places, and it is no instruction
        # s_branch / s_cbranch_* <signed word offset>: the offset is replaced by the target as objdump names it, symbol + byte
        # offset (the same symbol: "+0x..."), so a function that only moved -- or whose branches lead into code placed elsewhere
        # in the object -- compares equal, while a branch to another place in the function does not
        m = re.match(r'(s_c?branch\w*)\s+-?\d+$', ins)
        if m:
            t = re.search(r'<(.*)\+0x([0-9a-f]+)>\s*$', comment)
            ins = '%s %s' % (m.group(1), ('<+0x%s>' % t.group(2) if t.group(1) == cur else '<%s+0x%s>' % t.groups()) if t else '<?>')
        body = out[cur]
        # s_getpc_b64 s[a:b]; s_add_u32 sa, sa, <offset>; s_addc_u32 sb, sb, <hi>: a pc-relative address (a callee or constant
        # data), whose offset changes whenever the layout of the object does
        if len(body) >= 1 and body[-1].startswith('s_getpc_b64') and ins.startswith('s_add_u32'):
            ins = re.sub(r', [^,]+$', ', <pcrel>', ins)
        elif len(body) >= 2 and body[-2].startswith('s_getpc_b64') and ins.startswith('s_addc_u32'):
            ins = re.sub(r', [^,]+$', ', <pcrel>', ins)
        body.append(ins)
    return out


def side(arg):
    out = {}
    for co in arg.split(','):
        f = functions(co)
        dup = sorted(set(out) & set(f))
        if dup:
            sys.exit('%s: %s is defined in another object of this side too' % (co, dup[0]))
        out.update(f)
    return out


def main():
    a, b = side(sys.argv[1]), side(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else '.')
    bad = 0
    for name in sorted(set(a) | set(b)):
        if not pat.search(name):
            continue
        if name not in a or name not in b:
            print('%-100s only in %s' % (name[:100], 'b' if name not in a else 'a'))
            continue
        if a[name] == b[name]:
            print('%-100s same (%d instructions)' % (name[:100], len(a[name])))
        else:
            import difflib
            d = [l for l in difflib.unified_diff(a[name], b[name], lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
            d_code = [l for l in d if not l[1:].startswith(('s_branch', 's_cbranch'))]
            print('%-100s DIFFERS: %d lines (%d of them branches whose target moved)' % (name[:100], len(d), len(d) - len(d_code)))
            for l in (d_code or d)[:12]:
                print('      ' + l)
            bad += 1
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
