"""The oracle against Grok 9.2.0's recorded output (tests/golden/grok/, written by
tests/golden/make_grok_fixtures.py from Grok's own binaries): the pin that holds where no build of
Grok exists.  Encode: the oracle's bytes are Grok's.  Decode: the oracle's decode of that stream
under the recorded grk_decompress flags (-l, -r, -d, -t) equals Grok's, 9/7 included.
"""
import numpy as np
import pytest

import grok_cases as C

FX = C.load_fixtures()


def test_fixtures_are_the_chosen_cases():
    assert [f.name for f in FX] == [C.fixture_name(i) for i in range(len(C.FIXTURES))]
    assert [((f.key, f.flags), f.dflags) for f in FX] == C.FIXTURES
    flags = " ".join(f.flags for f in FX).split()
    for opt in "-n -b -c -I -r -M -t -X -S -E -q -p -d -T -P -L -u".split():
        assert opt in flags, opt
    dflags = " ".join(f.dflags for f in FX).split()
    for opt in "-l -r -d -t".split():
        assert opt in dflags, opt


@pytest.mark.parametrize("fx", FX, ids=[f.name for f in FX])
def test_oracle_encode_equals_recorded_grok(fx):
    assert C.oracle_encode(fx.key, fx.flags) == fx.cs


@pytest.mark.parametrize("fx", FX, ids=[f.name for f in FX])
def test_oracle_decode_equals_recorded_grok(fx):
    got = C.oracle_decode(fx.cs, fx.dflags, fx.flags)
    assert got.shape == fx.grok_decoded.shape
    np.testing.assert_array_equal(got, fx.grok_decoded)
