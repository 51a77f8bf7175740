"""CPU: system.CMAPTorsionForce on the host (openmmtools_amd/system.py, custom_expr.py, _engine.py) and the device's own arithmetic
compiled for the host (csrc/cmap_math.h, csrc/table2d_patch.h are plain C++): every refusal by its message, the accessors, the maps'
blocks, the interpolant at and between the nodes, the descriptor, the other interfaces, and the 70-term case of the GPU tests through
the device code without a GPU, held to tests/cmap_oracle.py."""
import copy
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cmap_oracle as oracle
from openmmtools_amd import alchemy, custom_expr as cx, states, testsystems, unit
from openmmtools_amd.system import System, system_to_desc, CMAPTorsionForce, CustomBondForce

TWO_PI = 2.0 * math.pi


def _system(n=10):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    return s


def _force(maps=oracle.MAPS[:1], torsions=((0, 0, 1, 2, 3, 1, 2, 3, 4),), periodic=False):
    f = CMAPTorsionForce()
    for size, energy in maps:
        f.addMap(size, energy)
    for row in torsions:
        f.addTorsion(*[int(v) for v in row])
    f.setUsesPeriodicBoundaryConditions(periodic)
    return f


def _desc(*forces, n=10):
    s = _system(n)
    for f in forces:
        s.addForce(f)
    return system_to_desc(s)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_force_and_the_item():
    f = CMAPTorsionForce()
    with pytest.raises(ValueError, match=r'CMAPTorsionForce: a map of size 1 \(at least 2\)'):
        f.addMap(1, [0.0])
    with pytest.raises(ValueError, match='CMAPTorsionForce: a map of size 4 needs 16 energies, not 15'):
        f.addMap(4, np.zeros(15))
    with pytest.raises(ValueError, match='a map energy that is not finite'):
        f.addMap(2, [0.0, 1.0, math.nan, 2.0])
    with pytest.raises(NotImplementedError, match=r'CMAPTorsionForce: a map of size 256 \(the engine takes 2 ... 255\)'):
        f.addMap(256, np.zeros(256 * 256))
    assert f.addMap(255, np.zeros(255 * 255)) == 0 and (255 + 1) ** 2 == cx.MAX_TABLE_CELLS
    with pytest.raises(ValueError, match='a map of size 3 needs 9 energies'):
        f.setMapParameters(0, 3, np.zeros(8))
    with pytest.raises(ValueError, match=r'the first dihedral \(0, 1, 2, 1\) names particle 1 twice'):
        f.addTorsion(0, 0, 1, 2, 1, 1, 2, 3, 4)
    with pytest.raises(ValueError, match=r'the second dihedral \(4, 2, 3, 4\) names particle 4 twice'):
        f.addTorsion(0, 0, 1, 2, 3, 4, 2, 3, 4)
    g = CMAPTorsionForce()
    for _ in range(64):
        g.addMap(2, np.zeros(4))
    with pytest.raises(NotImplementedError, match='CMAPTorsionForce: more than 64 maps in one force'):
        g.addMap(2, np.zeros(4))
    with pytest.raises(NotImplementedError, match='CMAPTorsionForce: changing a map or a torsion after set_system'):
        g.updateParametersInContext()
    # what only the System can tell
    with pytest.raises(ValueError, match=r'CMAPTorsionForce: torsion 0 names map 1 \(the force has 1\)'):
        _desc(_force(torsions=[(1, 0, 1, 2, 3, 1, 2, 3, 4)]))
    with pytest.raises(ValueError, match=r'CMAPTorsionForce: torsion 0 names map -1'):
        _desc(_force(torsions=[(-1, 0, 1, 2, 3, 1, 2, 3, 4)]))
    with pytest.raises(ValueError, match=r'CMAPTorsionForce: torsion 1 names particle 10 \(the System has 10\)'):
        _desc(_force(torsions=[(0, 0, 1, 2, 3, 1, 2, 3, 4), (0, 5, 6, 7, 8, 6, 7, 8, 10)]))
    with pytest.raises(ValueError, match='CMAPTorsionForce: torsion 0 names particle -2'):
        _desc(_force(torsions=[(0, 0, 1, 2, 3, 1, 2, 3, -2)]))
    with pytest.raises(ValueError, match='CMAPTorsionForce: 1 torsions but no map'):
        _desc(_force(maps=[]))
    crowd = [_force() for _ in range(8)] + [CustomBondForce('r')]
    with pytest.raises(NotImplementedError, match=r'9 custom forces in one System \(the engine takes 8\)'):
        _desc(*crowd)
    a, b = _force(), CustomBondForce('r')
    b.addBond(0, 1, []); b.setForceGroup(3)
    with pytest.raises(NotImplementedError, match='custom forces in several force groups'):
        _desc(a, b)
    assert 'custom_terms' not in _desc(_force(torsions=[]))                           # (maps without torsions: nothing to run)


def test_stores_pools_and_the_cpu_port_refuse_by_name():
    from openmmtools_amd import system_xml, _engine
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    s = _system(); s.addForce(_force())
    with pytest.raises(NotImplementedError, match='CMAPTorsionForce with the energy'):
        system_xml.to_xml(s)
    what = ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0)], [], [])
    # (layout='auto' asks exactly this: what it returns is what the sampler's warning names before it keeps the record container)
    assert what == "a System with a CMAPTorsionForce (energy %r)" % cx.CMAP_ENERGY_TEXT

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(s)
    with pytest.raises(NotImplementedError, match='CMAP torsion forces.*more than one compatibility group'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])
    here = os.path.dirname(os.path.abspath(__file__))
    cpu_lib = os.path.join(os.path.dirname(here), 'oracle', '_build', 'libremd_cpu.so')
    if not os.path.exists(cpu_lib):
        import __graft_entry__
        __graft_entry__.build()
    eng = _engine.HipEngine(lib_path=cpu_lib)
    al = testsystems.AlanineDipeptideVacuum()
    al.system.addForce(_force(torsions=[(0, 4, 6, 8, 14, 6, 8, 14, 16)]))
    with pytest.raises(NotImplementedError, match='remd_set_custom_terms.*CMAP torsion forces.*remd_hip_custom.h'):
        eng.set_system(system_to_desc(al.system))


# ---- API -------------------------------------------------------------------------------------------------------------------------------------
def test_accessors_round_trip():
    f = CMAPTorsionForce()
    e4 = np.arange(16.0)
    assert f.usesPeriodicBoundaryConditions() is False and f.getNumMaps() == 0 and f.getNumTorsions() == 0
    assert f.addMap(4, e4 * unit.kilojoule_per_mole) == 0 and f.addMap(2, [1.0, 2.0, 3.0, 4.0]) == 1 and f.getNumMaps() == 2
    assert f.getMapParameters(0) == (4, e4.tolist()) and f.getMapParameters(1) == (2, [1.0, 2.0, 3.0, 4.0])
    f.setMapParameters(1, 3, np.ones(9))
    assert f.getMapParameters(1) == (3, [1.0] * 9)
    assert f.addTorsion(1, 0, 1, 2, 3, 1, 2, 3, 4) == 0 and f.addTorsion(0, 5, 6, 7, 8, 9, 0, 1, 2) == 1 and f.getNumTorsions() == 2
    assert f.getTorsionParameters(1) == (0, 5, 6, 7, 8, 9, 0, 1, 2)
    f.setTorsionParameters(0, 0, 3, 2, 1, 0, 4, 3, 2, 1)
    assert f.getTorsionParameters(0) == (0, 3, 2, 1, 0, 4, 3, 2, 1)
    f.setUsesPeriodicBoundaryConditions(True); f.setForceGroup(7)
    assert f.usesPeriodicBoundaryConditions() is True and f.getForceGroup() == 7
    f.getMapParameters(0)[1][0] = 99.0                                              # (a copy: the force keeps its own)
    assert f.getMapParameters(0)[1][0] == 0.0
    g = copy.deepcopy(f)
    assert g.getTorsionParameters(1) == f.getTorsionParameters(1) and g.getMapParameters(1) == f.getMapParameters(1)


# ---- the maps' blocks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, 1, 2])
def test_a_maps_block_is_table2d_nodes_on_the_edge_repeated_grid(k):
    size, energy = oracle.MAPS[k]
    block = cx.cmap_block(size, energy)
    grid = oracle.edge_repeated(size, energy)
    assert block[:8].tolist() == [size + 1, size + 1, 0.0, TWO_PI, 0.0, TWO_PI, 1.0, 0.0] and len(block) == 8 + 4 * (size + 1) ** 2
    nodes = cx.table2d_nodes(size + 1, size + 1, grid, 0.0, TWO_PI, 0.0, TWO_PI, periodic=True)
    assert np.array_equal(block[8:], nodes.reshape(-1))
    assert np.array_equal(nodes[:size, :size, 0].reshape(-1), np.asarray(energy))    # energy[i + size*j] is node [j][i]
    assert np.array_equal(nodes[-1], nodes[0]) and np.array_equal(nodes[:, -1], nodes[:, 0])          # periodic in all four numbers
    ref = oracle.table(size, energy).nodes()                                        # the reference's dense solves: the same derivatives
    assert np.abs(nodes - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- the device's arithmetic on the host ---------------------------------------------------------------------------------------------------------
HOST_WRAPPER = '''
#include "cmap_math.h"
extern "C" void table2d(const double* B, double x, double y, double* out) { cst_table2d(B, x, y, out[0], out[1], out[2]); }
extern "C" double term(const double* B, const float* p, const double* box, double* F)
{
    float q[8][4]; cm3 G[8];
    for (int a = 0; a < 8; ++a) for (int c = 0; c < 4; ++c) q[a][c] = c < 3 ? p[3 * a + c] : 0.0f;
    const double v = cmap_term(B, q, box[0], box[1], box[2], G);
    for (int a = 0; a < 8; ++a) { F[3 * a] = G[a].x; F[3 * a + 1] = G[a].y; F[3 * a + 2] = G[a].z; }
    return v;
}
'''


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """csrc/cmap_math.h and csrc/table2d_patch.h compiled with the host compiler"""
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('cmap_host')
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'openmmtools_amd', 'csrc')
    (tmp / 'wrap.cpp').write_text(HOST_WRAPPER)
    lib_path = str(tmp / 'libcmaphost.so')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off', '-Wno-unknown-pragmas', '-I', csrc, str(tmp / 'wrap.cpp'), '-o', lib_path])
    lib = ctypes.CDLL(lib_path)
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    lib.table2d.argtypes = [dp, ctypes.c_double, ctypes.c_double, dp]
    lib.term.argtypes = [dp, fp, dp, dp]
    lib.term.restype = ctypes.c_double

    def table2d(block, x, y):
        out = np.zeros(3)
        lib.table2d(block.ctypes.data_as(dp), float(x), float(y), out.ctypes.data_as(dp))
        return out

    def term(block, x, box=(0.0, 0.0, 0.0)):
        p = np.ascontiguousarray(x, dtype=np.float32).reshape(24)
        b, F = np.array(box, dtype=np.float64), np.zeros(24)
        v = lib.term(block.ctypes.data_as(dp), p.ctypes.data_as(fp), b.ctypes.data_as(dp), F.ctypes.data_as(dp))
        return v, F.reshape(8, 3)
    return table2d, term


@pytest.mark.parametrize('k', [0, 1, 2])
def test_the_interpolant_returns_the_energies_at_the_nodes(host, k):
    """at every node (2 pi i / size, 2 pi j / size): energy[i + size*j] to 1e-13 relative, from the reference and from the device's
    patch on the package's block; the same one period on and one period back (the wrap)"""
    size, energy = oracle.MAPS[k]
    block, tab = cx.cmap_block(size, energy), oracle.table(size, energy)
    worst = 0.0
    for j in range(size):
        for i in range(size):
            want = energy[i + size * j]
            for shift in (0.0, TWO_PI, -TWO_PI):
                x, y = TWO_PI * i / size + shift, TWO_PI * j / size - shift
                for got in (tab.value_and_gradient(x, y)[0], host[0](block, x, y)[0]):
                    worst = max(worst, abs(got - want) / abs(want))
    print('size %d: worst relative deviation at a node %.3g' % (size, worst))
    assert worst <= 1e-13


def test_a_smooth_map_is_reproduced_to_the_splines_truncation_error(host):
    """f = cos(phi) + sin(2 psi) + cos(phi - psi) sampled at size = 24.  The interpolant is the tensor product of periodic cubic splines,
    whose 1D errors are |f - s| <= (5/384) h^4 max|f''''| and |f' - s'| <= (1/24) h^3 max|f''''| (Hall and Meyer 1976); for the tensor
    product, with c = 5/384 and d = 1/24: |f - S| <= c h^4 (max|d4f/dphi4| + max|d4f/dpsi4|) + c^2 h^8 max|d8f/dphi4 dpsi4|, and
    |df/dphi - dS/dphi| <= d h^3 max|d4f/dphi4| + c h^4 max|d5f/dphi dpsi4| + c d h^7 max|d8f/dphi4 dpsi4| (psi alike).  Here the
    maxima are 2 (phi^4), 17 (psi^4), 1 (every mixed one)."""
    size = 24
    a = TWO_PI * np.arange(size) / size
    phi, psi = a[None, :], a[:, None]
    energy = (np.cos(phi) + np.sin(2.0 * psi) + np.cos(phi - psi)).reshape(-1)
    block, tab = cx.cmap_block(size, energy), oracle.table(size, energy)
    h, c, d = TWO_PI / size, 5.0 / 384.0, 1.0 / 24.0
    bound_v = c * h ** 4 * (2.0 + 17.0) + c * c * h ** 8
    bound_x = d * h ** 3 * 2.0 + c * h ** 4 + c * d * h ** 7
    bound_y = d * h ** 3 * 17.0 + c * h ** 4 + c * d * h ** 7
    rng = np.random.default_rng(6)
    worst = np.zeros(3)
    for x, y in rng.uniform(-TWO_PI, 2.0 * TWO_PI, (400, 2)):
        want = np.array([math.cos(x) + math.sin(2.0 * y) + math.cos(x - y), -math.sin(x) - math.sin(x - y), 2.0 * math.cos(2.0 * y) + math.sin(x - y)])
        for got in (np.array(tab.value_and_gradient(x, y)), host[0](block, x, y)):
            worst = np.maximum(worst, np.abs(got - want))
    print('worst / bound: value %.3g / %.3g, d/dphi %.3g / %.3g, d/dpsi %.3g / %.3g' % (worst[0], bound_v, worst[1], bound_x, worst[2], bound_y))
    assert worst[0] <= bound_v and worst[1] <= bound_x and worst[2] <= bound_y
    assert worst[0] > 1e-3 * bound_v                                                # (the bound is of the error's own size, not slack)


def test_the_seventy_term_case_through_the_device_code_on_the_host(host):
    """every term of the GPU tests' 70-term case (both replicas) through cmap_term as the kernel calls it: energy within 1e-11 of the
    reference per term, each of the eight forces within 1e-11 of the term's largest -- f64 against f64, before any rounding to f32 -- and
    the same with minimum images on the straddling term"""
    blocks = [cx.cmap_block(size, energy) for size, energy in oracle.MAPS]
    worst_e = worst_f = 0.0
    for x in oracle.XS70:
        ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, x)
        for t, row in enumerate(oracle.TORSIONS70):
            v, F = host[1](blocks[row[0]], x[row[1:]])
            worst_e = max(worst_e, abs(v - ref['E'][t]) / abs(ref['E'][t]))
            worst_f = max(worst_f, np.abs(F - ref['G'][t]).max() / np.abs(ref['G'][t]).max())
    boxes, xs = oracle.straddling_positions()
    for periodic in (True, False):
        ref = oracle.evaluate([oracle.MAPS[2]], [(0, 0, 1, 2, 3, 4, 5, 6, 7)], xs[0], boxes[0], periodic)
        v, F = host[1](blocks[2], xs[0], boxes[0] if periodic else (0.0, 0.0, 0.0))
        worst_e = max(worst_e, abs(v - ref['E'][0]) / abs(ref['E'][0]))
        worst_f = max(worst_f, np.abs(F - ref['G'][0]).max() / np.abs(ref['G'][0]).max())
    print('device code on the host: worst relative energy deviation %.3g, force %.3g' % (worst_e, worst_f))
    assert worst_e <= 1e-11 and worst_f <= 1e-11
    # a collinear quadruple: finite, the documented convention (the force on the collinear triple's end particle exactly zero)
    x = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.25, 0.0, 0.0], [0.25, 0.125, 0.0], [0.375, 0.125, 0.125]])
    v, F = host[1](blocks[1], x[[0, 1, 2, 3, 1, 2, 3, 4]])
    want_v, want_F, phi, _ = oracle.convention_term(oracle.table(*oracle.MAPS[1]), x[[0, 1, 2, 3, 1, 2, 3, 4]])
    assert phi == 0.0 and math.isfinite(v) and np.isfinite(F).all() and not F[0].any() and np.abs(F[1:]).max() > 0.1
    assert abs(v - want_v) <= 1e-13 * abs(want_v) and np.abs(F - want_F).max() <= 1e-13 * np.abs(want_F).max()


def test_the_stand_alone_host_program_is_clean_under_the_sanitizers(tmp_path):
    """tools/cmap_host_check.cpp, a program with its own main, built with -fsanitize=address,undefined: the 70-term case (both
    replicas) through cmap_term against the reference, then huge, infinite and NaN arguments of cst_table2d; exit status 0 means
    agreement within 1e-11 and no sanitizer report"""
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blocks = [cx.cmap_block(size, energy) for size, energy in oracle.MAPS]
    with open(tmp_path / 'case.bin', 'wb') as f:
        np.array([len(b) for b in blocks], dtype=np.int32).tofile(f)
        for b in blocks:
            b.tofile(f)
        oracle.TORSIONS70.astype(np.int32).tofile(f)
        oracle.XS70.astype(np.float32).tofile(f)
        for x in oracle.XS70:
            ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, x)
            ref['E'].tofile(f); ref['G'].tofile(f)
    exe = str(tmp_path / 'cmap_host_check')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wno-unknown-pragmas',
                           '-I', os.path.join(root, 'openmmtools_amd', 'csrc'), os.path.join(root, 'tools', 'cmap_host_check.cpp'), '-o', exe])
    done = subprocess.run([exe, str(tmp_path / 'case.bin')], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0 and '140 terms' in done.stdout and 'ERROR' not in done.stderr and 'runtime error' not in done.stderr


# ---- the descriptor and the other interfaces -------------------------------------------------------------------------------------------------
def test_the_descriptor():
    from openmmtools_amd import _engine
    f = _force(maps=oracle.MAPS, torsions=oracle.TORSIONS70, periodic=True)
    f.setForceGroup(4)
    t = _desc(f, n=74)['custom_terms']
    assert list(t) == ['000']
    t = t['000']
    assert t['kind'] == cx.KIND_CMAP == 8 and t['n_particles'] == 8 and t['atoms'].shape == (70, 8) and t['atoms'].dtype == np.int32
    assert np.array_equal(t['atoms'], oracle.TORSIONS70[:, 1:]) and np.array_equal(t['map_index'], oracle.TORSIONS70[:, 0]) and t['map_index'].dtype == np.int32
    sizes = [8 + 4 * (s + 1) ** 2 for s, _ in oracle.MAPS]
    assert t['map_offsets'].tolist() == [0, sizes[0], sizes[0] + sizes[1]] and len(t['consts']) == sum(sizes)
    for (size, energy), off in zip(oracle.MAPS, t['map_offsets']):
        assert np.array_equal(t['consts'][off:off + 8 + 4 * (size + 1) ** 2], cx.cmap_block(size, energy))
    assert t['program'].shape == (0, 2) and t['params'].shape == (70, 0) and t['stack_depth'] == 0 and len(t['global_defaults']) == 0
    assert t['periodic'] == 1 and t['force_group'] == 4
    # the struct: the fields of the CMAP kind behind those of the collective variables, as in include/remd_hip_custom.h
    assert _engine.RemdCustomForceDescCMAP._fields_ == [('map_index', _engine.c_int32_p), ('n_maps', _engine.C.c_int32), ('map_offsets', _engine.c_int32_p)]
    assert issubclass(_engine.RemdCustomForceDescCMAP, _engine.RemdCustomForceDesc)
    assert _engine.RemdCustomForceDescCMAP.map_index.offset == _engine.C.sizeof(_engine.RemdCustomForceDesc)
    # beside a force with globals: the handle's columns in every entry, none of them the map's
    b = CustomBondForce('k*r'); b.addGlobalParameter('k', 2.0); b.addBond(0, 1, [])
    both = _desc(b, _force())['custom_terms']
    assert [e['kind'] for e in both.values()] == [cx.KIND_BOND, cx.KIND_CMAP] and both['001']['global_names'] == ['k']
    sk = _system(); sk.addForce(b); sk.addForce(_force())
    assert np.array_equal(cx.custom_globals(sk, ['k'], [object()]), [[2.0]])          # (the map has no globals to look up)


def test_a_changed_map_is_another_system():
    s1, s2, s3 = _system(), _system(), _system()
    s1.addForce(_force()); s2.addForce(_force())
    e = oracle.MAPS[0][1].copy(); e[5] += 1e-9
    s3.addForce(_force(maps=[(4, e)]))
    assert s1.fingerprint() == s2.fingerprint() != s3.fingerprint()


def test_the_alchemical_factory_passes_the_force_through():
    al = testsystems.AlanineDipeptideVacuum()
    f = _force(maps=oracle.MAPS[1:], torsions=[(1, 4, 6, 8, 14, 6, 8, 14, 16)])
    al.system.addForce(f)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [h for h in system.getForces() if isinstance(h, CMAPTorsionForce)]
    assert len(kept) == 1 and kept[0].getNumMaps() == 2 and kept[0].getTorsionParameters(0) == (1, 4, 6, 8, 14, 6, 8, 14, 16)
    assert kept[0].getMapParameters(1) == f.getMapParameters(1)
    assert [t['kind'] for t in system_to_desc(system)['custom_terms'].values()] == [cx.KIND_CMAP]
