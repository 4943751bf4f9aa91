"""CPU: the work split of gemm_nt_wreg_kernel (csrc/gemm_nt_wreg_split.h) as a host program under the address and
undefined-behaviour sanitizers (tools/wreg_split_host_check.cpp, a stand-alone program with its own main), and the host-only
predicate of the entry."""
import os
import re
import shutil
import subprocess

from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_covers_every_unit_once(tmp_path):
    """Every (group, 16-row unit) exactly once, contiguous shares inside one group, shares of a group within one unit of each other,
    and the longest share of 66,560 rows over 256 (255) workgroups within 5 % of the mean - over 65,536 / 66,560 / 73,800 / 24,576
    rows x {1, 2, 3, 16} groups x {255, 256} workgroups, the row counts of tests/test_gpu_gemm_wreg.py and its few-workgroup cases."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'wreg_split_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'wreg_split_host_check.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r'wreg_split_host_check ok: \d+ cases', out.stdout), out.stdout[-2000:] + out.stderr[-2000:]
    line = re.search(r'M +66560 groups +1 workgroups 256: grid 256, shares (\d+)\.\.(\d+) units \(mean ([\d.]+)\)', out.stdout)
    assert line and (int(line.group(1)), int(line.group(2)), float(line.group(3))) == (16, 17, 16.25)


def test_entry_validates_before_any_launch(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    ok = lib.vited_gemm_nt_wreg_supported
    assert ok(384, 384, 384, 65536, 1, 1, 0) == 1
    assert ok(384, 384, 768, 66560, 16, 2, 66560 * 768) == 1           # the decoder's stacked kv projection
    assert ok(392, 384, 1152, 65536, 3, 3, 0) == 1                     # qkv as three groups
    assert ok(384, 384, 384, 0, 1, 1, 0) == 0 and ok(384, 384, 384, 1 << 31, 1, 1, 0) == 0
    assert ok(383, 384, 384, 16, 1, 1, 0) == 0 and ok(384, 380, 384, 16, 1, 1, 0) == 0     # rows shorter than K
    assert ok(388, 384, 384, 16, 1, 1, 0) == 0                         # 16-byte pieces need strides in multiples of 8
    assert ok(384, 384, 384, 16, 2, 2, 0) == 0                         # two groups side by side need ldo >= 768
    assert ok(384, 384, 768, 16, 0, 1, 0) == 0 and ok(384, 384, 768, 16, 2, 0, 0) == 0
    BAD_ARG, UNSUPPORTED = 1, 2
    call = lib.vited_gemm_nt_wreg
    assert call(None, 384, 16, 384, None, 16, 384, 16, 1, 1, 0, 0, None) == BAD_ARG
    assert call(16, 384, 16, 384, None, 16, 384, 16, 1, 1, 0, -1, None) == BAD_ARG
    assert call(16, 384, 16, 384, None, 16, 380, 16, 1, 1, 0, 0, None) == UNSUPPORTED
    assert call(16, 384, 24, 384, None, 16, 384, 16, 1, 1, 0, 0, None) == BAD_ARG          # W not 16-byte aligned
    select = lib.vited_gemm_nt_wreg_select
    assert select(2) == BAD_ARG and select(1) == 0 and select(0) == 1 and select(0) == 0
