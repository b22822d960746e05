#!/usr/bin/env python3
"""device_code_diff.py - are the gfx950 kernels of two builds of the library the same machine code?  For a change that claims to leave the device side alone.
Per kernel of the hipcc code object: demangled name, instruction text (addresses and `//` comments stripped) and the register counts, LDS, scratch and
kernarg sizes of the code-object metadata; the embedded assembly band code object is compared byte for byte.  A trailing template argument that the change
removed from a kernel is dropped from the names of the `before` side with --drop-last-arg <kernel name>.
usage: device_code_diff.py before.so after.so [--drop-last-arg ls_estimate_ringb_kernel]     exit status 1 on any difference"""
import hashlib, os, re, subprocess, sys, tempfile
from opsel_census import LLVM, code_objects

KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_segment_size', 'max_flat_workgroup_size')


def tool(name, *args):
    exe = os.path.join(LLVM, name)
    return subprocess.run([exe if os.path.exists(exe) else name] + list(args), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True, check=True).stdout


def kernels(so, drop):
    """{demangled kernel name: (instruction text, metadata)} of the hipcc code object, and the sha256 of every embedded assembly code object"""
    out, blobs = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            if os.path.basename(co).startswith('asm'):
                blobs.append(hashlib.sha256(open(co, 'rb').read()).hexdigest())
                continue
            meta = {}
            for item in re.split(r'\n  - ', tool('llvm-readelf', '--notes', co).split('amdhsa.kernels:')[1].split('\namdhsa.target')[0])[1:]:
                f = dict(re.findall(r'^ {0,4}\.(\w+): +(.*)$', item, re.M))
                meta[f['name']] = tuple((k, f.get(k)) for k in KEYS)
            cur, text = None, {}
            for line in tool('llvm-objdump', '-d', '--mcpu=gfx950', co).splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
                if m: cur = m.group(1); text[cur] = []
                elif cur and line.strip(): text[cur].append(line.split('//')[0].strip())
            names = sorted(n for n in text if n in meta)
            for n, dem in zip(names, tool('c++filt', *names).splitlines()):
                if drop and re.match(r'^(void )?(\w+::)*' + re.escape(drop) + '<', dem):
                    dem = re.sub(r', [^,<>]+>\(', '>(', dem, count=1)
                assert dem not in out, dem
                out[dem] = ('\n'.join(text[n]).replace(n, dem), meta[n])
    return out, blobs


if __name__ == '__main__':
    drop = sys.argv[sys.argv.index('--drop-last-arg') + 1] if '--drop-last-arg' in sys.argv else None
    (ka, ba), (kb, bb) = kernels(sys.argv[1], drop), kernels(sys.argv[2], None)
    bad = ['only in %s: %s' % (w, n) for w, s in (('before', set(ka) - set(kb)), ('after', set(kb) - set(ka))) for n in sorted(s)]
    for n in sorted(set(ka) & set(kb)):
        if ka[n][1] != kb[n][1]: bad.append('metadata differs: %s\n    %s\n    %s' % (n, ka[n][1], kb[n][1]))
        if ka[n][0] != kb[n][0]: bad.append('instructions differ: %s' % n)
    if ba != bb: bad.append('embedded assembly code objects differ: %s / %s' % (ba, bb))
    for w, p in (('before', sys.argv[1]), ('after', sys.argv[2])):
        print('%s sha256 %s  %s' % (w, hashlib.sha256(open(p, 'rb').read()).hexdigest(), p))
    print('kernels: %d before, %d after, %d compared (%d instructions); embedded assembly code objects: %d, %s' % (
        len(ka), len(kb), len(set(ka) & set(kb)), sum(v[0].count('\n') + 1 for v in kb.values()), len(bb), 'byte-identical' if ba == bb else 'DIFFERENT'))
    print('differences: %d' % len(bad))
    for b in bad: print('  ' + b)
    sys.exit(1 if bad else 0)
