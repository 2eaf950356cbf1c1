"""CPU-only checks of the build's unit list against the sources (no kernel runs, nothing is compiled by these tests themselves): every translation unit
under csrc/ is built exactly once, the geometry units cannot lose the flags their bit-exactness depends on, and every C ABI function of the binding is
defined in exactly one unit."""
import os
import re

from matryodshka_amd import build


def _units_on_disk():
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp")))


def _text(unit):
    with open(os.path.join(build.CSRC, unit)) as f:
        return f.read()


def test_every_source_is_built_exactly_once():
    listed = [src for src, _ in build.SOURCES]
    assert sorted(listed) == sorted(set(listed)), "a unit is listed twice in build.SOURCES"
    assert sorted(listed) == _units_on_disk()
    for family in (build.GEO_UNITS, build.CNN_UNITS):
        assert set(family) <= set(listed)


def test_geometry_units_are_compiled_without_contraction():
    flags = dict(build.SOURCES)
    including = [u for u in _units_on_disk() if re.search(r'^\s*#\s*include\s+"geometry_device\.h"', _text(u), re.M)]
    assert sorted(including) == sorted(build.GEO_UNITS)
    for unit in including:
        assert "-ffp-contract=off" in flags[unit], unit


def test_every_hip_unit_is_compiled_without_the_slp_vectorizer():
    for unit, flags in build.SOURCES:
        if unit.endswith(".hip"):
            assert "-fno-slp-vectorize" in flags, unit


def test_every_abi_function_is_defined_in_exactly_one_unit(native_lib):
    texts = {u: _text(u) for u in _units_on_disk()}
    for name in native_lib.SIGNATURES:
        # a definition at the start of a line: return type, name, opening parenthesis
        pattern = re.compile(r'^(?:extern "C" )?(?:int|int32_t|uint32_t|size_t|void|const char \*)\s*%s\(' % re.escape(name), re.M)
        hits = [u for u, t in texts.items() if pattern.search(t)]
        assert len(hits) == 1, "%s: defined in %s" % (name, hits or "no unit")
        assert len(pattern.findall(texts[hits[0]])) == 1, "%s: more than once in %s" % (name, hits[0])


def test_the_single_geometry_file_is_gone():
    assert not os.path.exists(os.path.join(build.CSRC, "geometry.hip"))
