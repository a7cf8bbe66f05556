"""The recipe that builds the reference's own kernels for gfx950 (oracle/ref_gpu.py): with a reference checkout it leaves both
libraries, exporting the driver's entry points, and a second call compiles nothing; without one it returns and touches nothing;
and nothing under oracle/_ref/ is tracked.  No GPU: the libraries are never loaded here, their symbol tables are read from the file."""
import os
import shutil
import struct
import subprocess

import pytest

from oracle import ref_gpu as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REFERENCE = rg._reference_sources(rg.reference_dir()) is not None


def dynamic_symbols(path):
    """Names defined in the .dynsym of a little-endian ELF64 shared object."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = set()
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 11:      # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for o in range(offset, offset + size, entsize):
            st_name, _, _, st_shndx = struct.unpack_from("<IBBH", data, o)
            if st_shndx != 0:  # defined here
                out.add(data[str_off + st_name:data.index(b"\0", str_off + st_name)].decode())
    return out


def _tree(path):
    if not os.path.isdir(path):
        return None
    return sorted((os.path.join(d, n), os.stat(os.path.join(d, n)).st_mtime_ns) for d, _, names in os.walk(path) for n in names)


@pytest.mark.skipif(not HAVE_REFERENCE, reason="no reference checkout (MOM_REFERENCE_DIR): nothing to build from")
def test_build_leaves_both_libraries_and_a_second_call_compiles_nothing():
    assert rg.build() is True
    for variant in rg.VARIANTS:
        assert rg.available(variant), variant
        syms = dynamic_symbols(rg.lib_path(variant))
        assert set(rg.ENTRY_POINTS) <= syms, sorted(set(rg.ENTRY_POINTS) - syms)
        # ... over the reference's own entry points, linked into the same library
        for method in ("markVisible", "forward", "backward"):
            assert any("CudaRasterizer" in s and "Rasterizer" in s and method in s for s in syms), method
        assert any("SimpleKNN" in s and "knn" in s for s in syms)
    before = _tree(rg.OUT)
    assert rg.build() is True
    assert _tree(rg.OUT) == before
    assert rg.compiler_version()


def test_build_without_a_checkout_returns_and_touches_nothing(tmp_path, monkeypatch):
    before = _tree(rg.OUT)
    monkeypatch.setenv("MOM_REFERENCE_DIR", str(tmp_path / "no_such_checkout"))
    assert rg.build() is False
    assert rg.build(force=True) is False
    assert _tree(rg.OUT) == before


def test_nothing_under_the_build_directory_is_tracked():
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in [line.strip() for line in f]
    git = shutil.which("git")
    if git and os.path.exists(os.path.join(ROOT, ".git")):
        r = subprocess.run([git, "-C", ROOT, "ls-files", "--", "oracle/_ref"], capture_output=True, text=True, check=True)
        assert r.stdout.strip() == "", r.stdout
    # no copy of a reference source beside the recipe either: it holds the driver, the redirecting headers and the record
    kinds = {os.path.splitext(n)[1] for _, _, names in os.walk(rg.RECIPE) for n in names}
    assert ".cu" not in kinds and kinds <= {".h", ".cuh", ".cpp", ".md"}, kinds
