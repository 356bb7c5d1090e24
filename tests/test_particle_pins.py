"""CPU tier: the numpy statement of the rain-particle model (tools/particles.py) still produces the pinned bits.

tests/golden/particle_pins.json holds SHA-256 digests of what the statement returned on the commit named in
tests/golden/make_particle_pins.py; this test recomputes them with the current code.  The other host tests assert numpy == g++
(and the GPU tests device == numpy): together with this one they tie all three statements to those bits."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def test_numpy_statement_has_the_pinned_bits(built):
    spec = importlib.util.spec_from_file_location('make_particle_pins', os.path.join(GOLDEN, 'make_particle_pins.py'))
    pins = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pins)
    with open(os.path.join(GOLDEN, 'particle_pins.json')) as fh:
        want = json.load(fh)
    got = pins.digests()
    assert sorted(got) == sorted(want)
    bad = sorted(k for k in want if got[k] != want[k])
    assert bad == [], bad
    assert len(want) > 150
