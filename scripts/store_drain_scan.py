"""Where a kernel waits for its own stores: a static scan of the gfx950 assembly of rainhip.hip (hipcc -S with the product's
flags; no GPU needed).  On this hardware generation vmcnt counts vector loads AND stores, so a vector load issued behind a store
and waited for with `s_waitcnt vmcnt(0)` also waits for that store's acknowledgement: a memory round trip the kernel did not ask
for.  The usual source is a field of a descriptor in global memory read through a plain reference: behind every store the
compiler has to fetch it again (see k_composite32's header, profiles/compositor_epilogue_cost.md).

  python scripts/store_drain_scan.py [--asm FILE | --source FILE] [--all] [--tail KERNEL] [kernel name fragments ...]

Per kernel (those with a finding, or all with --all / those named): the number of vector stores, and every vector load that
follows a store in the text with no `vmcnt(0)` wait between them and is then waited for with `vmcnt(0)`.  For k_composite32
(or --tail KERNEL) also the instructions between the kernel's last barrier and its end.  The scan follows the TEXT of the
assembly, not its control flow: it is a reading aid, to be followed by reading the lines it names."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'rain-rendering_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# the product's device flags (__graft_entry__.HIP_FLAGS) less what links
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-Wno-unused-value', '-Wno-unused-result']

STORE = re.compile(r'^(global|flat|buffer)_(store|atomic)\w*')
VLOAD = re.compile(r'^(global|flat|buffer)_load\w*')
SLOAD = re.compile(r'^s_(buffer_)?load\w*')
VMCNT = re.compile(r'^s_waitcnt\b.*\bvmcnt\((\d+)\)')


def assembly(source=None, extra=()):
    """The device assembly of `source` (default: the library's rainhip.hip) as text."""
    source = source or os.path.join(CSRC, 'rainhip.hip')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'rainhip.s')
        subprocess.check_call([HIPCC] + FLAGS + list(extra) + ['-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '--cuda-device-only', '-S',
                               source, '-o', out], stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(asm):
    """{mangled name: [(line number, instruction text)]} of every kernel: labels stay in as 'name:' entries."""
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M))
    out, cur = {}, None
    for no, line in enumerate(asm.split('\n'), 1):
        s = line.split(';')[0].strip()
        if not s:
            continue
        if s.endswith(':') and s[:-1] in names:
            cur = out.setdefault(s[:-1], [])
            continue
        if cur is None:
            continue
        if s.startswith('.Lfunc_end'):
            cur = None
            continue
        if s.startswith('.') and not s.endswith(':'):
            continue                                   # a directive
        cur.append((no, s))
    return out


def demangle(names):
    names = list(names)
    txt = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n')
    short = {}
    for n, d in zip(names, txt):
        d = re.sub(r'\(anonymous namespace\)::', '', d)
        d = re.sub(r'^void ', '', d)
        short[n] = re.sub(r'\((?!.*<).*', '', d) if '<' not in d else re.sub(r'>\(.*', '>', d)
    return short


def scan(body):
    """(number of vector stores, [(load line, load text, wait line)]): the loads issued behind a store that a vmcnt(0) waits for."""
    stores, found, pending_store, pending_loads = 0, [], False, []
    for no, s in body:
        if STORE.match(s):
            stores += 1
            pending_store = True
        elif VLOAD.match(s):
            if pending_store:
                pending_loads.append((no, s))
        else:
            m = VMCNT.match(s)
            if m and int(m.group(1)) == 0:
                found += [(ln, ls, no) for ln, ls in pending_loads]
                pending_store, pending_loads = False, []
    return stores, found


def tail(body):
    """The instructions from behind the kernel's last s_barrier to its end."""
    last = max([k for k, (_, s) in enumerate(body) if s.startswith('s_barrier')] or [-1])
    return body[last + 1:]


def after_first_store(body):
    """The instructions from the kernel's first vector store to its end."""
    first = min([k for k, (_, s) in enumerate(body) if STORE.match(s)] or [len(body)])
    return body[first:]


def epilogue_report(body):
    """What a store burst must not hold, counted from the kernel's first store to its end: vector loads, scalar loads, and
    waits that name vmcnt."""
    rest = after_first_store(body)
    return {'stores': [x for x in rest if STORE.match(x[1])],
            'vector_loads': [x for x in rest if VLOAD.match(x[1])],
            'scalar_loads': [x for x in rest if SLOAD.match(x[1])],
            'vmcnt_waits': [x for x in rest if VMCNT.match(x[1])]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--asm', help='an assembly file made earlier, instead of compiling')
    ap.add_argument('--source', help='another rainhip.hip (e.g. the parent commit\'s)')
    ap.add_argument('--all', action='store_true', help='every kernel, not only those with a finding')
    ap.add_argument('--tail', default='k_composite32', help='the kernel whose text behind its last barrier is printed')
    ap.add_argument('names', nargs='*', help='only kernels whose demangled name holds one of these')
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else assembly(a.source)
    ks = kernels(asm)
    short = demangle(ks)
    print('%-60s %6s %s' % ('kernel', 'stores', 'loads behind a store, waited for with vmcnt(0)'))
    for n in sorted(ks, key=lambda n: short[n]):
        if a.names and not any(f in short[n] for f in a.names):
            continue
        stores, found = scan(ks[n])
        if not (found or a.all or a.names):
            continue
        print('%-60s %6d %d' % (short[n][:60], stores, len(found)))
        for ln, ls, wn in found:
            print('    line %d: %s        (waited for at line %d)' % (ln, ls, wn))
    for n in sorted(ks, key=lambda n: short[n]):
        if re.sub(r'<.*', '', short[n]) != a.tail:
            continue
        r = epilogue_report(ks[n])
        print('\n%s, from its first store to its end: %d stores, %d vector loads, %d scalar loads, %d waits naming vmcnt' %
              (short[n], len(r['stores']), len(r['vector_loads']), len(r['scalar_loads']), len(r['vmcnt_waits'])))
        print('%s behind its last barrier:' % short[n])
        for no, s in tail(ks[n]):
            print('  %7d  %s' % (no, s))


if __name__ == '__main__':
    main()
