"""The listed terms against the bits recorded from the commit before the kernels with energies moved onto csrc/listed_terms.h
(tests/listed_terms_bits.py, tests/golden/listed_terms_bits.npz): each class alone and together in force-only evaluations, in both
organisations of the listed launch; the kernels with energies, their nine components and the kick that takes their forces; the
alchemical exception and exclusion factors; the three places the listed workgroups run; the resident kernel; the softened bonded terms
of general alchemical regions.  The arithmetic is meant to be the recorded commit's, product for product, so every bit has to come back."""
import pytest
import listed_terms_bits as ltb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', ltb.CASES)
def test_listed_terms_reproduce_the_recorded_bits(hip_engine_factory, case):
    ltb.assert_same_bits(getattr(ltb, case)(hip_engine_factory), case)
