"""The keys of the pinned bits, checked without a GPU.  The pin tests skip under a key their stores do not hold -- right
for another toolchain, wrong for an edit of bullet-envs_amd/build.py that moved a stamp's name or text by a byte: every pin
would then skip on the GPU and nothing would say so.  Here the texts of the default build's stamps are computed from
build.py's own functions (no compile; `hipcc --version` alone) and each family's key must be in its store."""
import json
import os

import pytest

import bit_pins
from bit_pins import build_py

# hipcc's version lines under which the stores' keys were computed, and those keys
PINNED_TOOLCHAIN = ("HIP version: 7.2.26015-fc0010cf6a | AMD clang version 22.0.0git (https://github.com/RadeonOpenCompute/"
                    "llvm-project roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5)")
PINNED_KEYS = {"step": "6e946590e810", "query": "22ff1c4c058f", "dynamics": "9a2269098dde"}


@pytest.fixture(scope="module")
def stamps():
    """[(file, text)] of what a default build leaves next to the library"""
    return build_py.stamp_texts()


def test_the_stamps_names(stamps):
    names = ("libsnk.so.toolchain", "libsnk.so.cmd", "libsnk.so.render.cmd", "libsnk.so.world.cmd", "libsnk.so.dyn.cmd")
    assert build_py.STAMPS == names
    assert tuple(os.path.relpath(path, bit_pins.PKGDIR) for path, _ in stamps) == names
    assert build_py.SOURCES == ("csrc/snk_api.hip", "csrc/snk_render.hip", "csrc/snk_world.hip", "csrc/snk_dyn.hip")
    assert sorted(bit_pins.FAMILIES) == sorted(PINNED_KEYS)


@pytest.mark.parametrize("family", sorted(PINNED_KEYS))
def test_the_default_builds_key_is_pinned(stamps, family):
    key, txt = bit_pins.key([text for _, text in stamps][:bit_pins.FAMILIES[family].stamps])
    pinned = json.load(open(bit_pins.store(family)))
    assert key in pinned, "the %s pins would skip on the GPU: no key %s in %s (it hashes %r)" % (
        family, key, bit_pins.FAMILIES[family].store, txt)
    assert pinned[key]["built_by"] == txt.replace("\n", " || ")
    # a library that lies next to the package is the one the GPU tests will load: its stamps must be these texts
    if os.path.exists(build_py.LIB):
        for path, text in stamps[:bit_pins.FAMILIES[family].stamps]:
            assert open(path).read() == text, path
        assert bit_pins.built_key(family) == (key, txt)


@pytest.mark.parametrize("family", sorted(PINNED_KEYS))
def test_the_keys_are_those_of_the_pinning_toolchain(stamps, family):
    if stamps[0][1] != PINNED_TOOLCHAIN:
        pytest.skip("another hipcc (%s): its keys are checked for presence only" % stamps[0][1])
    assert bit_pins.key([text for _, text in stamps][:bit_pins.FAMILIES[family].stamps])[0] == PINNED_KEYS[family]
