"""Kernel resources and instruction streams of two source trees, side by side: "parent | this commit".

    python tools/kernel_resources.py PARENT_TREE THIS_TREE vi_basis.hip vi_eval.hip ... [--edited REGEX ...] [--work DIR] [--reuse]

Every unit named is compiled in each tree that has it (a unit may exist in one tree only: kernels are matched across all
units by their mangled names) with the command `make -n` prints for its object file, device pass only, as assembly with
-Rpass-analysis=kernel-resource-usage.  Per kernel the table has VGPRs, AGPRs, SGPRs, scratch, static LDS and occupancy of
both trees and a verdict on the instruction stream: the assembly of the kernel with directives, comments, labels and blank
lines dropped (and the counters taken out of the local labels an instruction names - .LBB<function>_, .Lpost_getpc<n> -, which
follow the kernel's place in the file) is compared line by line.  A kernel whose demangled name matches an --edited pattern was changed on purpose: it must use
no scratch where the parent has none and keep the parent's occupancy; every other kernel must be instruction-identical.
Runs on the CPU only; it compares and does nothing else.  Exit status 1 if a kernel misses its gate."""
import argparse
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

FIELDS = [('VGPRs', 'VGPRs'), ('AGPRs', 'AGPRs'), ('SGPRs', 'TotalSGPRs'), ('scratch', 'ScratchSize [bytes/lane]'),
          ('LDS', 'LDS Size [bytes/block]'), ('occupancy', 'Occupancy [waves/SIMD]')]


def compile_unit(tree, unit, work, reuse):
    """-> (assembly path, report path, seconds) of the device pass of `unit` in `tree`"""
    csrc = os.path.join(tree, 'volumetricinterp_amd', 'csrc')
    stem = os.path.join(work, os.path.splitext(unit)[0])
    asm, rpt, tim = stem + '.s', stem + '.rpt', stem + '.time'
    if reuse and all(os.path.exists(p) for p in (asm, rpt, tim)):
        return asm, rpt, float(open(tim).read().split()[1])
    obj = os.path.splitext(unit)[0] + '.o'
    lines = subprocess.check_output(['make', '-C', csrc, '-n', '-B', obj], text=True).splitlines()
    cmd = next(l for l in lines if ' -c ' in l and unit in l).split()
    cmd = cmd[:cmd.index('-o')]
    cmd[cmd.index('-c')] = '--cuda-device-only'
    cmd += ['-S', '-Rpass-analysis=kernel-resource-usage', '-o', asm]
    t0 = time.time()
    with open(rpt, 'w') as fh:
        subprocess.check_call(cmd, cwd=csrc, stdout=fh, stderr=subprocess.STDOUT)
    dt = time.time() - t0
    with open(tim, 'w') as fh:
        fh.write('%s %.0f s\n' % (os.path.splitext(unit)[0], dt))
    return asm, rpt, dt


def read_report(path):
    """-> {mangled name: {field: int}}"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark:\s+(.+?): (\d+) \[-Rpass', line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def read_streams(path, names):
    """-> {mangled name: [instruction lines]} for the kernels `names`"""
    out, cur = {}, None
    for line in open(path):
        line = line.split(';')[0].strip()
        if not line:
            continue
        if line.endswith(':'):
            if line[:-1] in names:
                cur = out.setdefault(line[:-1], [])
            continue
        if line.startswith('.'):
            if line.startswith('.end_amdhsa_kernel') or line.startswith('.section'):
                cur = None
            continue
        if cur is not None:
            cur.append(re.sub(r'\.LBB\d+_|\.Lpost_getpc\d+', lambda m: m.group(0).rstrip('0123456789_'), ' '.join(line.split())))
    return out


def demangle(names):
    names = list(names)
    for tool in ('/opt/rocm/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt'):
        try:
            res = subprocess.check_output([tool], input='\n'.join(names), text=True).splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
        pretty = [re.sub(r'^void ', '', r).replace('(anonymous namespace)::', '') for r in res]
        return {n: re.sub(r'\(.*\)$', '', p) if '<' in p else p.split('(')[0] for n, p in zip(names, pretty)}
    return {n: n for n in names}


def tree_side(pool, tree, units, work, reuse):
    """starts the compilations of one tree on `pool`; -> a function that waits for them and reads the results"""
    os.makedirs(work, exist_ok=True)
    have = [u for u in units if os.path.exists(os.path.join(tree, 'volumetricinterp_amd', 'csrc', u))]
    futures = [pool.submit(compile_unit, tree, u, work, reuse) for u in have]
    return lambda: read_side(have, [f.result() for f in futures])


def read_side(have, done):
    res, streams, where, times = {}, {}, {}, {}
    for u, (asm, rpt, dt) in zip(have, done):
        r = read_report(rpt)
        res.update(r)
        streams.update(read_streams(asm, set(r)))
        where.update({k: u for k in r})
        times[u] = dt
    return res, streams, where, times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('parent')
    ap.add_argument('this')
    ap.add_argument('units', nargs='+')
    ap.add_argument('--edited', nargs='*', default=[], help='regular expressions: kernels changed on purpose')
    ap.add_argument('--work', default='kernel_resources_work', help='directory for the assembly and the reports')
    ap.add_argument('--reuse', action='store_true', help='take what --work already holds instead of compiling')
    ap.add_argument('--jobs', type=int, default=4)
    a = ap.parse_args()
    with ThreadPoolExecutor(a.jobs) as pool:        # the units of both trees share the pool
        sides = [tree_side(pool, t, a.units, os.path.join(a.work, d), a.reuse) for t, d in ((a.parent, 'parent'), (a.this, 'this'))]
        (pr, ps, pw, pt), (nr, ns, nw, nt) = [wait() for wait in sides]
    names = demangle(set(pr) | set(nr))
    print('Kernel resource usage for gfx950, parent commit | this commit: the object file\'s command of the Makefile, device pass '
          'only, with -S -Rpass-analysis=kernel-resource-usage.')
    print('Columns: VGPRs AGPRs SGPRs scratch[bytes/lane] static-LDS[bytes] occupancy[waves/SIMD]; the dynamic LDS is set at '
          'launch.  Then the unit(s) and the verdict on the instruction stream, with the count of instructions.')
    print('Device pass alone, seconds: parent ' + ', '.join('%s %.0f' % kv for kv in pt.items()) + ' | this commit ' +
          ', '.join('%s %.0f' % kv for kv in nt.items()))
    fmt = lambda r: ' '.join(str(r[k]) for _, k in FIELDS) if r else '-'
    bad = same = 0
    for n in sorted(set(pr) | set(nr), key=lambda n: names[n]):
        p, q = pr.get(n), nr.get(n)
        unit = pw.get(n, '-') if pw.get(n) == nw.get(n) else '%s -> %s' % (pw.get(n, '-'), nw.get(n, '-'))
        if p is None or q is None:
            verdict = 'ONLY IN ' + ('THIS COMMIT' if p is None else 'THE PARENT')
            bad += 1
        elif ps.get(n) == ns.get(n):
            verdict = 'identical (%d)' % len(ns[n])
            same += 1
        elif any(re.search(e, names[n]) for e in a.edited):
            ok = (q['ScratchSize [bytes/lane]'] == 0 or p['ScratchSize [bytes/lane]'] > 0) and \
                q['Occupancy [waves/SIMD]'] >= p['Occupancy [waves/SIMD]']
            verdict = 'edited (%d -> %d): %s' % (len(ps[n]), len(ns[n]), 'within its gate' if ok else 'MISSES ITS GATE')
            bad += not ok
        else:
            verdict = 'DIFFERS (%d -> %d)' % (len(ps[n]), len(ns[n]))
            bad += 1
        print('  %-40s %-19s | %-19s %s: %s' % (names[n], fmt(p), fmt(q), unit.replace('.hip', ''), verdict))
    print('%d kernels in the parent, %d in this commit, %d in both; %d instruction-identical, %d miss the gate.' % (
        len(pr), len(nr), len(set(pr) & set(nr)), same, bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
