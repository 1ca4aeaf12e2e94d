"""The register budget of the kernel k_extremum_sph, from the compiler's resource report (no GPU needed)."""
import os
import re
import shutil
import subprocess

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_extremum_sph_registers(tmp_path):
    """hipcc's resource report of csrc/vi_extremum.hip (device pass, the Makefile's flags): three instantiations of the kernel -
    the orders (6, 4), (12, 8), (2, 12) - and nothing else in the unit; no scratch at (6, 4) or at (2, 12).  The search keeps
    x, the best point and the step (3 doubles each), the best value and gradient norm and the trust length across the walk; the
    start and the radius are read again after it.  At (12, 8) the gradient kernel already sits at 256 VGPRs, so the figures
    there are printed, not pinned (profiles/r29_kernel_resources.txt has them all)."""
    csrc = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc')
    # the command the Makefile has for the unit's object file (make -n prints it), so that the pin follows its flags
    make = ['make', '-C', csrc, '-n', '-B', 'vi_extremum.o']
    if os.environ.get('HIPCC') or not os.path.exists('/opt/rocm/bin/hipcc'):
        make.append('HIPCC=' + (os.environ.get('HIPCC') or shutil.which('hipcc') or 'hipcc'))
    lines = subprocess.run(make, capture_output=True, text=True, check=True).stdout.splitlines()
    cmd = next(l for l in lines if ' -c vi_extremum.hip' in l).split()
    assert '-O3' in cmd and '--offload-arch=gfx950' in cmd, cmd
    cmd = cmd[:cmd.index('-o')] + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'ext.o')]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    use = {}
    name = None
    for l in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            name = m.group(1)
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)', l)
        if m and name:
            use.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
    for n, u in sorted(use.items()):
        print(n, u)
    kernel = 'k_extremum_sphILi'
    mine = {n: u for n, u in use.items() if kernel in n}
    assert len(mine) == 3, sorted(use)
    pinned = {n: u for n, u in mine.items() if kernel + '6ELi4E' in n or kernel + '2ELi12E' in n}
    assert len(pinned) == 2, sorted(mine)
    for n, u in pinned.items():
        assert u['ScratchSize'] == 0, (n, u)
    assert len(use) == 3, sorted(use)
