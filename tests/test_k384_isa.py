"""The counted vmcnt waits of gemm_nt_areg_kernel (csrc/gemm_nt_k384.hip) are right only while hipcc emits exactly 8 global stores
(16 under the GELU' epilogue) for one item's epilogue and spills nothing: `make check-k384` reads that off the ISA of every
instance the product build compiles.  Needs hipcc, not a GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vit-ed_amd', 'csrc')


def test_epilogue_store_count_behind_the_counted_waits():
    r = subprocess.run(['make', '-C', CSRC, 'check-k384', 'ARCH=gfx950'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'check-k384 ok: 2 instances' in r.stdout, r.stdout[-2000:]
