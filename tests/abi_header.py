"""What the ABI tests (test_header_abi.py, test_*_abi.py) share: the declarations of a C header, the ctypes type of a parameter and
the build script as a module."""

import ctypes
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

_SCALARS = {'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float, 'uint32_t': ctypes.c_uint32}


def declarations(header_path):
    """{name: (return type, [parameter declarations])}"""
    text = re.sub(r'/\*.*?\*/', '', Path(header_path).read_text(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(tdk_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text, flags=re.S):
        args = ' '.join(args.split())
        out[name] = (ret, [] if args in ('', 'void') else [a.strip() for a in args.split(',')])
    return out


def ctype_of(decl):
    """The ctypes type of one parameter declaration: every pointer and the stream handle travel as c_void_p."""
    if '*' in decl or decl.startswith('tdk_stream_t'):
        return ctypes.c_void_p
    assert decl.split()[0] in _SCALARS, decl
    return _SCALARS[decl.split()[0]]


def load_build_module():
    spec = importlib.util.spec_from_file_location('tdk_build_for_test', ROOT / 'torch-darktable_amd' / 'build.py')
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build

