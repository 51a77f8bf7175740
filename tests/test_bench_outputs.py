"""bench.py --dump-outputs: what the last timed iteration handed to its caller, written as float64 .npy files.  No GPU here: the
headline sampler runs a few MD steps on libremd_cpu.so (the same C ABI), twice from the same seed, and the dumps must agree."""
import os
import numpy as np
import oracle
import bench
from openmmtools_amd._engine import HipEngine

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')


def _dump(directory, R=4, md_steps=2):
    if not os.path.exists(CPU_LIB):
        oracle.build()
    eng = HipEngine(lib_path=CPU_LIB)
    eng.is_device = False
    try:
        sampler, ts = bench.build_sampler(R, eng, None, md_steps)
        sampler.run(2)
        bench.dump_outputs(str(directory), sampler)
    finally:
        eng.close()
    return {f[:-4]: np.load(os.path.join(str(directory), f)) for f in os.listdir(str(directory))}, ts.system.getNumParticles()


def test_dump_outputs_are_the_iterations_results_and_repeat(tmp_path):
    a, n_atoms = _dump(tmp_path / 'a')
    b, _ = _dump(tmp_path / 'b')
    R = 4
    shapes = dict(replica_index=(R,), replica_thermodynamic_states=(R,), energy_thermodynamic_states=(R, R), n_accepted_matrix=(R, R),
                  n_proposed_matrix=(R, R), positions=(R, n_atoms, 3), velocities=(R, n_atoms, 3), box_vectors=(R, 3, 3))
    assert {k: v.shape for k, v in a.items()} == shapes
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert sorted(a['replica_thermodynamic_states']) == list(range(R)) and a['n_proposed_matrix'].sum() > 0
    assert list(a['replica_index']) == list(range(R))
    for k in shapes:
        assert np.array_equal(a[k], b[k]), k


def test_a_large_dump_keeps_a_seeded_sample_of_the_replicas(tmp_path, monkeypatch):
    """Past the byte budget of the coordinates, a fixed sample of the replicas is written (the same one every run)."""
    monkeypatch.setattr(bench, 'DUMP_COORDINATE_BYTES', 2 * 2 * 8 * 3 * 2269)          # two replicas of alanine dipeptide in water
    a, n_atoms = _dump(tmp_path / 'a')
    b, _ = _dump(tmp_path / 'b')
    assert a['positions'].shape == a['velocities'].shape == (2, n_atoms, 3) and a['box_vectors'].shape == (2, 3, 3)
    assert a['energy_thermodynamic_states'].shape == (4, 4)
    idx = list(a['replica_index'])
    assert len(idx) == 2 and idx == sorted(set(idx)) and set(idx) <= set(range(4))
    assert all(np.array_equal(a[k], b[k]) for k in a)
