"""The direct-space pair path of csrc/forces.hip against the bits recorded from the commit before its host side was reorganised
(tests/pair_path_bits.py, tests/golden/pair_path_bits.npz): the split path of an Ewald run with and without an alchemical ladder,
through a re-sort and a change of the replica count; the one-system path; the tile kernel on the sorted buffers; the split path of a
reaction-field run; two blocks of replicas.  The kernels are the recorded commit's to the byte, so every bit has to come back: a
difference is a wrong kernel argument, allocation or launch order on the host side, not rounding."""
import pytest
import pair_path_bits as ppb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', ppb.CASES)
def test_pair_path_reproduces_the_recorded_bits(hip_engine_factory, case):
    ppb.assert_same_bits(getattr(ppb, case)(hip_engine_factory), case)
