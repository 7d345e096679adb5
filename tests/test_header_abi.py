"""CPU-only: what holds for every public header alike, once per row of the registry torch_darktable._native.HEADERS -- the library
exports what the header declares and answers its version, the hand-written ctypes table mirrors the header parameter for parameter
and shares no name with another table, and the header is part of the build's source hash.  The registry, build.HEADERS and the
headers on disk are the same set.  What is particular to one header (its names, parameter lists, constants, formulas) is in that
header's own test_*_abi.py."""

import ctypes
from pathlib import Path

import pytest

from abi_header import ctype_of, declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / 'include'
FILES = sorted(p.name for p in INCLUDE.glob('tdk_hip*.h'))   # the cases are the headers on disk: one that nothing else lists still gets tested
# abi_header.declarations reads the int and size_t functions only: of tdk_hip.h it misses tdk_last_error (const char*) and
# tdk_profile_report (int64_t), and its table takes types ctype_of does not derive (c_char_p, c_uint, POINTER(c_float)).
# tests/test_abi.py holds that table to the header by names and parameter counts instead.
PARSED = [f for f in FILES if f != 'tdk_hip.h']


def row(file):
    from torch_darktable import _native

    return next(r for r in _native.HEADERS if r[0] == file)


def test_registry_build_list_and_disk_hold_the_same_headers(td):
    from torch_darktable import _native

    build = load_build_module()
    assert [r[0] for r in _native.HEADERS] == [h.name for h in build.HEADERS]   # the same order too
    assert all(h.parent == INCLUDE for h in build.HEADERS)
    assert sorted(h.name for h in build.HEADERS) == FILES   # a header on disk that is not hashed fails here
    assert _native.ALL_SIGNATURES == tuple(r[1] for r in _native.HEADERS)
    assert _native.ABI_VERSIONS == {r[2]: (r[3], r[4]) for r in _native.HEADERS}


@pytest.mark.parametrize('file', FILES)
def test_header_is_part_of_the_source_hash(file):
    build = load_build_module()
    assert INCLUDE / file in build.HEADERS and INCLUDE / file in build._inputs()
    assert (INCLUDE / file).exists()


@pytest.mark.parametrize('file', FILES)
def test_library_answers_the_version_of_the_registry(td, file):
    _, table, version_fn, expected, _ = row(file)
    assert version_fn in table
    lib = ctypes.CDLL(str(ROOT / 'torch-darktable_amd' / 'torch_darktable' / 'libtdk_hip.so'))
    getattr(lib, version_fn).restype = ctypes.c_int
    assert getattr(lib, version_fn)() == expected


@pytest.mark.parametrize('file', PARSED)
def test_library_exports_every_declared_symbol(td, file):
    lib = ctypes.CDLL(str(ROOT / 'torch-darktable_amd' / 'torch_darktable' / 'libtdk_hip.so'))
    for name in declarations(INCLUDE / file):
        assert hasattr(lib, name), f'{name} declared in {file} but not exported'


@pytest.mark.parametrize('file', PARSED)
def test_ctypes_table_matches_header(td, file):
    from torch_darktable import _native

    table = row(file)[1]
    decls = declarations(INCLUDE / file)
    assert sorted(table) == sorted(decls)
    assert not set(table) & set().union(*(t for t in _native.ALL_SIGNATURES if t is not table))
    for name, (restype, argtypes) in table.items():
        ret, params = decls[name]
        assert restype is (ctypes.c_int if ret == 'int' else ctypes.c_size_t), name
        assert [ctype_of(p) for p in params] == list(argtypes), f'{name}: header {params}, ctypes {argtypes}'
        assert getattr(_native.lib, name).argtypes == list(argtypes)
