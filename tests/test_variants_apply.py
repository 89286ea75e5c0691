"""Every variant of tools/variants.py still applies to the sources (CPU, no compile).

The A/B tool patches prismdb_amd/csrc by exact text: each substitution must
match exactly once in the file as the variant's earlier substitutions left
it, or `variants.py build` stops -- which nobody learns before they are on a
GPU box with a variant that no longer builds.  The same rule is applied here
to in-memory copies of the sources.  Out of reach without a build or another
checkout, and skipped: "@src" variants (another checkout's sources) and what
follows an "@git" substitution (a whole file from history) in that file.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prismdb_amd", "csrc")


def _load():
    spec = importlib.util.spec_from_file_location("prismdb_tools_variants", os.path.join(ROOT, "tools", "variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VARIANTS = _load().VARIANTS


@pytest.fixture(scope="module")
def sources():
    out = {}
    for f in os.listdir(CSRC):
        with open(os.path.join(CSRC, f)) as fh:
            out[f] = fh.read()
    return out


def test_there_are_variants():
    assert "base" in VARIANTS and VARIANTS["base"] == [] and len(VARIANTS) > 50


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_every_substitution_matches_exactly_once(sources, name):
    spec = VARIANTS[name]
    if spec and spec[0][0] == "@src":
        assert all(s[0] != "@src" for s in spec[1:])
        return
    text = dict(sources)  # this variant's copy (strings: the shared ones stay as read)
    replaced = set()      # files an "@git" substitution took from history
    for fname, old, new in spec:
        assert fname in text, (name, fname)
        if old == "@git":
            replaced.add(fname)
            continue
        if fname in replaced:
            continue
        assert isinstance(new, str) and old != new and old != "", (name, fname)
        assert text[fname].count(old) == 1, (name, fname, text[fname].count(old), old[:80])
        text[fname] = text[fname].replace(old, new)
