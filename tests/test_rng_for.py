"""The seeded inputs of tests/ are the same in every process: util.rng_for derives a generator from the crc32 of its key's
text.  Built on the built-in hash instead (salted per process for str), every run and every xdist worker would draw other
inputs, and a failure could not be reproduced from its test id."""
import numpy as np

from . import util as U


def test_rng_for_first_draw_is_pinned():
    """The first draw for one (seed, key) against a literal: a return to the built-in hash, or any other formula, fails
    here in any process."""
    assert int(U.rng_for(U.kRandomSeed, "a", np.int8, 3).integers(0, 2**63)) == 1194124408917585352
