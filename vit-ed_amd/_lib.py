"""ctypes binding of libvited_hip.so (the C ABI declared in include/vited.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent,
importing the ops raises, and every op raises ``RuntimeError`` for tensors that are not on a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VITED_LIB') or os.path.join(_HERE, 'libvited_hip.so')  # VITED_LIB: kernel-experiment builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'vited.h')

F32, BF16, F16 = 0, 1, 2
I32, I64 = 3, 4
EPI_STORE, EPI_GELU, EPI_RESIDUAL, EPI_MUL_GELU_GRAD, EPI_STORE_F32, EPI_MUL, EPI_GELU_GRAD = 0, 1, 2, 3, 4, 5, 6
B_NK, B_KN = 0, 1

_lib = None


class VitedLibraryError(RuntimeError):
    pass


def header_declared_functions():
    """Names of every function include/vited.h declares (used by the ABI test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(vited_[a-z0-9_]+)\s*\(', text)))


_C_SCALARS = {'int': C.c_int, 'int64_t': C.c_int64, 'float': C.c_float}
_PROTOTYPE = re.compile(r'(\w[\w\s*]*?)\s*\b(vited_\w+)\s*\(([^)]*)\)\s*;')


def _ctype(decl: str, where: str, scalars: dict):
    """ctypes type of a C type of the header: every pointer is a c_void_p, the scalars map one to one."""
    if '*' in decl:
        return C.c_void_p
    try:
        return scalars[' '.join(decl.split())]
    except KeyError:
        raise VitedLibraryError(f'include/vited.h: {where} has the C type {decl.strip()!r}, which the binding cannot express') from None


def parse_signatures(text: str, scalars: dict | None = None) -> dict:
    """name -> (restype, argtypes) of every ``vited_*`` prototype in ``text`` (the source of include/vited.h).  ``scalars``: the
    by-value C types accepted (default: ``int``, ``int64_t``, ``float``)."""
    scalars = _C_SCALARS if scalars is None else scalars
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        ret = ' '.join(ret.replace('*', ' *').split())
        restype = C.c_char_p if ret == 'const char *' else _ctype(ret, f'the return of {name}', scalars)
        argtypes = []
        if params.strip() != 'void':
            for i, param in enumerate(params.split(',')):
                decl = re.sub(r'\b\w+\s*$', '', param)          # drop the parameter's name
                argtypes.append(_ctype(decl, f'parameter {i} ({" ".join(param.split())}) of {name}', scalars))
        sigs[name] = (restype, argtypes)
    missed = set(re.findall(r'\b(vited_\w+)\s*\(', text)) - set(sigs)
    if missed:
        raise VitedLibraryError(f'include/vited.h: cannot parse the prototypes of {sorted(missed)}')
    return sigs


# name -> (restype, argtypes), derived from include/vited.h: the header is the only statement of each signature
# the header itself also passes one double by value (vited_mine_pairs' neg_per_pos: Python's float, undiminished)
SIGNATURES = parse_signatures(open(HEADER_PATH).read(), {**_C_SCALARS, 'double': C.c_double})


def load():
    """Load the shared library (once) and attach the signatures.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitedLibraryError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C vit-ed_amd/csrc`.  There is no CPU or PyTorch fallback for the ViT-ED hot path.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise VitedLibraryError(f'{LIB_PATH} does not export {name} (stale build?)') from e
        fn.restype = res
        fn.argtypes = args
    if lib.vited_abi_version() != 1:
        raise VitedLibraryError(f'ABI version mismatch: library {lib.vited_abi_version()}, binding 1')
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().vited_strerror(code).decode()
        raise RuntimeError(f'{what} failed: {msg} (vited error {code})')


def call(name: str, *args):
    """Call the status-returning entry ``name`` and raise ``RuntimeError`` unless it returned VITED_OK."""
    check(getattr(load(), name)(*args), name)
