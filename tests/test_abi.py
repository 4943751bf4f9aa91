"""CPU: the C-ABI shared library loads and exports every symbol include/vited.h declares, and the ctypes binding derived
from the header has the header's types.  No compute call is made (there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ensure_built(vited):
    if not os.path.exists(vited._lib.LIB_PATH):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'vit-ed_amd', 'csrc'), '-j', '8'], check=True)


def test_header_binding_and_library_agree(vited):
    _ensure_built(vited)
    declared = vited._lib.header_declared_functions()
    assert declared == sorted(vited._lib.SIGNATURES), 'include/vited.h and the ctypes SIGNATURES table differ'
    lib = ctypes.CDLL(vited._lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f'{name} is declared in include/vited.h but not exported'
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if ' T vited_' in l)
    assert exported == declared, 'exported vited_* symbols differ from the header'


def test_library_loads_and_reports_errors(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    assert lib.vited_abi_version() == 1
    assert lib.vited_strerror(0) == b'ok' and b'workspace' in lib.vited_strerror(4) and b'unknown' in lib.vited_strerror(99)
    # argument validation happens before any launch, so these are safe without a GPU
    assert lib.vited_gemm(None, 0, None, 0, 0, 1, 0, 0, 0, 0, None, None, None, None, None, 0, 0, 0, 0, 0, None) == 1
    assert lib.vited_layernorm_fwd(None, 0, None, None, None, 1, 0, None, None, 0, 0, 1e-6, None) == 1
    assert lib.vited_linear_bwd_weight_workspace_bytes(65536, 1152, 384) > 0
    assert lib.vited_last_gemm_path() == 0
    with pytest.raises(RuntimeError, match=r'^vited_gemm failed: .+ \(vited error 1\)$'):
        vited._lib.call('vited_gemm', None, 0, None, 0, 0, 1, 0, 0, 0, 0, None, None, None, None, None, 0, 0, 0, 0, 0, None)


def _header_text(vited):
    return open(vited._lib.HEADER_PATH).read()


def test_signatures_have_the_header_types(vited):
    sigs, C = vited._lib.SIGNATURES, ctypes
    text = re.sub(r'/\*.*?\*/', ' ', _header_text(vited), flags=re.S)
    prototypes = re.findall(r'\b(vited_\w+)\s*\(([^)]*)\)', text)
    assert sorted(name for name, _ in prototypes) == sorted(sigs)
    for name, params in prototypes:
        assert len(sigs[name][1]) == (0 if params.strip() == 'void' else params.count(',') + 1), name
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert sigs['vited_abi_version'] == (i, [])
    assert sigs['vited_strerror'] == (C.c_char_p, [i])
    assert sigs['vited_gemm'] == (i, [p, i64, p, i64, i, i, i64, i64, i64, i, p, p, p, p, p, i64, i64, i64, i64, i, p])
    assert sigs['vited_layernorm_fwd'][1][11] is f                       # eps
    assert sigs['vited_linear_bwd_weight_workspace_bytes'] == (i64, [i64, i64, i64])
    assert sigs['vited_fold_context_weights'][1][1] is p                 # const float* const* w


def test_prototype_parser(vited):
    L, C = vited._lib, ctypes
    assert L.parse_signatures('#define VITED_X 1\n/* int vited_gone(int a); */\nint64_t vited_probe(int a, const float* const* b,\n'
                              '    float c,   // a comment\n    uint8_t *d);') == {'vited_probe': (C.c_int64, [C.c_int, C.c_void_p, C.c_float,
                                                                                                        C.c_void_p])}
    with pytest.raises(L.VitedLibraryError, match=r'parameter 1 \(double x\) of vited_probe .*\'double\''):
        L.parse_signatures('int vited_probe(const void* p, double x, void* stream);')
    with pytest.raises(L.VitedLibraryError, match=r'return of vited_probe .*\'unsigned\''):
        L.parse_signatures('unsigned vited_probe(void);')
    with pytest.raises(L.VitedLibraryError, match='vited_probe'):
        L.parse_signatures('int vited_probe(int (*callback)(int));')


def test_named_constants_match_the_header(vited):
    defines = {k: int(v) for k, v in re.findall(r'^#define VITED_(\w+) (-?\d+)', _header_text(vited), flags=re.M)}
    names = ['F32', 'BF16', 'F16', 'I32', 'I64', 'EPI_STORE', 'EPI_GELU', 'EPI_RESIDUAL', 'EPI_MUL_GELU_GRAD', 'EPI_STORE_F32', 'EPI_MUL',
             'EPI_GELU_GRAD', 'B_NK', 'B_KN']
    assert {k for k in defines if k != 'OK' and not k.startswith(('ERR_', 'ABI_'))} == set(names)
    for name in names:
        assert getattr(vited._lib, name) == defines[name], name
    assert defines['ABI_VERSION'] == 1                                   # what load() requires


def test_host_arrays(vited):
    t = torch.ones(4)
    ptrs = vited.ops._host_array(ctypes.c_void_p, [None, t])
    assert ptrs._type_ is ctypes.c_void_p and list(ptrs) == [None, t.data_ptr()]
    assert list(vited.ops._host_array(ctypes.c_float, [0.5], 3)) == [0.5, 0.0, 0.0]
    assert list(vited.ops._host_array(ctypes.c_int, map(int, (True, False)))) == [1, 0]


def test_row_complete_kernel_tile_heights(vited):
    """gemm_row.hip picks the tile height (96 / 128 / 144 / 160 rows) with the smallest makespan over rounds of 256 workgroups;
    the partial-rows query (= number of tiles, one [2][384] partial each) shows the choice without a GPU."""
    _ensure_built(vited)
    lib = vited._lib.load()
    rows = lib.vited_linear_layernorm_bwd_partial_rows
    assert rows(65536) == 512          # 64-token batches of 1024: two full rounds of 128-row tiles
    assert rows(66560) == 463          # 65-token batches: 144-row tiles (two rounds; 520 x 128 would need three)
    assert rows(72 * 1025) == 462      # config H decoder, 72 pairs: 160-row tiles (two rounds; 577 x 128 would need three)
    assert rows(24 * 1024) == 256      # config H encoder, 24 images: one round of 96-row tiles
    assert rows(100) == 2              # 96 + 4 rows
    assert lib.vited_linear_layernorm_supported(4096, 384, 384) == 1
    assert lib.vited_linear_layernorm_supported(4096, 384, 96) == 0      # the contraction comes in K = 64 tiles
    assert lib.vited_linear_layernorm_supported(4096, 512, 384) == 0     # rows are 384 wide
    assert lib.vited_linear_layernorm_bwd_workspace_bytes(65536, 384) == 512 * 2 * 384 * 4
