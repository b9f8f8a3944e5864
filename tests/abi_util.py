"""What a native library's public header declares, and the one check that a library, its header and its prototype table in
pixelsynth_amd._lib agree (used by test_abi.py and the CPU tests of the libraries beside libpixelsynth_hip.so)."""
import os
import re
import subprocess

from pixelsynth_amd import _lib, _libraries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(header, line_comments=True):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", txt) if line_comments else txt


def header_symbols(name="pixelsynth_hip.h"):
    return sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", _text(name, line_comments=False))))


def header_prototypes(headers=("pixelsynth_hip.h", "pixelsynth_hip_debug.h")):
    """{name: [parameter text]} of every prototype of the headers (comments stripped)."""
    protos = {}
    for name in headers:
        for fn, params in re.findall(r"\b(ps_[a-z0-9_]+)\s*\(([^;{)]*)\)\s*;", _text(name)):
            protos[fn] = [p.strip() for p in params.split(",")] if params.strip() not in ("", "void") else []
    return protos


def ends_in_stream(protos):
    return {n for n, p in protos.items() if p and re.fullmatch(r"void\s*\*\s*stream", p[-1])}


def assert_library_matches_header(library):
    """The library `library` of _libraries.LIBRARIES: its prototype table names the entry points its header(s) declare, each with as
    many arguments; the entries marked STREAM are exactly the prototypes that end in `void *stream` (the ones call() appends the
    current stream to), and no other argument is one; the loaded .so exports exactly that set of the ps_ namespace.
    -> the header's prototypes"""
    entry = next(e for e in _libraries.LIBRARIES if e.name == library)
    table, protos = _lib.PROTOS[library], header_prototypes(entry.headers)
    assert set(protos) == set(table), set(protos) ^ set(table)
    assert entry.last_error in table
    for name, (_, args) in table.items():
        assert len(args) == len(protos[name]), (name, len(args), protos[name])
    assert {n for n, (_, args) in table.items() if args and args[-1] is _lib.STREAM} == ends_in_stream(protos)
    assert all(a is not _lib.STREAM for _, args in table.values() for a in args[:-1])
    L = _lib.library(library)
    for name in protos:
        assert hasattr(L, name), f"{name} declared in include/ but not exported"
    out = subprocess.run(["nm", "-D", "--defined-only", _libraries.path(entry)], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ps_")}
    assert exported == set(protos), exported ^ set(protos)
    return protos
