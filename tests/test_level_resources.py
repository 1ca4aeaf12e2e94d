"""The register budget of the level-crossing kernel k_level_sph, from the compiler's resource report (no GPU needed)."""
import os
import re
import shutil
import subprocess

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_level_sph_registers(tmp_path):
    """hipcc's resource report of csrc/vi_level.hip (device pass, the Makefile's flags): three instantiations of k_level_sph -
    the orders (6, 4), (12, 8), (2, 12) -, the two column kernels of the crossing maps and nothing else in the unit; neither
    (6, 4) nor (2, 12) nor a column kernel uses scratch.  At (12, 8) the gradient kernel already sits at 256 VGPRs, so the
    figures there are printed, not pinned (profiles/r27_kernel_resources.txt has them all)."""
    csrc = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc')
    # the command the Makefile has for the unit's object file (make -n prints it), so that the pin follows its flags
    make = ['make', '-C', csrc, '-n', '-B', 'vi_level.o']
    if os.environ.get('HIPCC') or not os.path.exists('/opt/rocm/bin/hipcc'):
        make.append('HIPCC=' + (os.environ.get('HIPCC') or shutil.which('hipcc') or 'hipcc'))
    lines = subprocess.run(make, capture_output=True, text=True, check=True).stdout.splitlines()
    cmd = next(l for l in lines if ' -c vi_level.hip' in l).split()
    assert '-O3' in cmd and '--offload-arch=gfx950' in cmd, cmd
    cmd = cmd[:cmd.index('-o')] + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'level.o')]
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
    level = {n: u for n, u in use.items() if 'k_level_sphILi' in n}
    columns = {n: u for n, u in use.items() if 'k_cross_columns' in n}
    for n, u in sorted(use.items()):
        print(n, u)
    assert len(level) == 3 and len(columns) == 2 and len(use) == 5, sorted(use)
    pinned = {n: u for n, u in level.items() if 'k_level_sphILi6ELi4E' in n or 'k_level_sphILi2ELi12E' in n}
    assert len(pinned) == 2, sorted(level)
    pinned.update(columns)
    for n, u in pinned.items():
        assert u['ScratchSize'] == 0, (n, u)
