"""The output bits of every entry that walks the FULL packets of finished launches, against the
digests tests/golden/packet_bits.json holds (tests/golden/make_packet_bits.py wrote them with the
library as it was before these entries came to share their tile walk, wave merge and launch turn).
Their sums have a fixed order, so a digest that differs is a changed result, not noise."""
import json
import os

import pytest

import packet_bits_cases as PB
from packets_fixture import torch  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'packet_bits.json')


def test_every_output_array_has_the_recorded_bits(torch):
    with open(GOLDEN) as f:
        want = json.load(f)
    eng, res, one, table = PB.make_world(torch)
    got = PB.digests(PB.run(eng, res, one, table))
    eng.close()
    assert sorted(got) == sorted(want), 'the calls are not the recorded ones'
    differ = [name for name in got if got[name] != want[name]]        # in the order of the calls
    assert not differ, f'{len(differ)} of {len(got)} arrays differ, the first: {differ[0]}'
