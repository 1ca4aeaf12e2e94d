"""The register budget of the tiled evaluation kernel k_eval_sph_fast, from the compiler's resource report (no GPU needed)."""
import os
import re
import shutil
import subprocess

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_eval_sph_fast_registers(tmp_path):
    """hipcc's resource report of csrc/vi_eval.hip (device pass, the Makefile's flags): no k_eval_sph_fast instantiation uses
    scratch, and k_eval_sph_fast<6, 4, 1, double> - the default order at a tile of one timestep - stays within 96 VGPRs, five
    waves per SIMD: the figure the comments at fast_chains (vi_chain_device.h) and bench.py's roofline entry rest on
    (95 when this test was written)."""
    csrc = os.path.join(REPO_ROOT, 'volumetricinterp_amd', 'csrc')
    # the command the Makefile has for the unit's object file (make -n prints it), so that the pin follows its flags
    make = ['make', '-C', csrc, '-n', '-B', 'vi_eval.o']
    if os.environ.get('HIPCC') or not os.path.exists('/opt/rocm/bin/hipcc'):
        make.append('HIPCC=' + (os.environ.get('HIPCC') or shutil.which('hipcc') or 'hipcc'))
    lines = subprocess.run(make, capture_output=True, text=True, check=True).stdout.splitlines()
    cmd = next(l for l in lines if ' -c vi_eval.hip' in l).split()
    assert '-O3' in cmd and '--offload-arch=gfx950' in cmd, cmd
    cmd = cmd[:cmd.index('-o')] + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'k2.o')]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    use = {}
    name = None
    for l in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            name = m.group(1)
        m = re.search(r'remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)', l)
        if m and name:
            use.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
    fast = {n: u for n, u in use.items() if 'k_eval_sph_fastILi' in n}
    for n, u in sorted(fast.items()):
        print(n, u)
    # seven orders x tiles of 16, 4, 1 with fp64 chains, two orders x three tiles with fp32 chains
    assert len(fast) == 27, sorted(use)
    for n, u in fast.items():
        assert u['ScratchSize'] == 0, (n, u)
    default = [u for n, u in fast.items() if 'k_eval_sph_fastILi6ELi4ELi1EdEE' in n]
    assert len(default) == 1, sorted(fast)
    assert default[0]['VGPRs'] <= 96, default[0]
