"""Iterations/s of the single-GPU share of the other BASELINE configs, same engine and protocol as
bench.py: config 2 (LJ fluid 512, 16 lambda_sterics states), config 4 share (CB7:B2 host-guest, 8 replicas per GPU out
of 64 alchemical states), config 5 share (DHFR, 16 replicas per GPU out of 128 states, SAMS global jump).
Prints one JSON line per config.  (The headline config 3 is bench.py.)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from openmmtools_amd import testsystems, states, mcmc, unit, alchemy
from openmmtools_amd.multistate import ReplicaExchangeSampler, SAMSSampler, ParallelTemperingSampler
from openmmtools_amd._engine import HipEngine


def alchemical_states(system, atoms, lam_e, lam_s, T=300.0):
    region = alchemy.AlchemicalRegion(alchemical_atoms=atoms)
    asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(system, region)
    out = []
    for le, ls in zip(lam_e, lam_s):
        a = states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le)
        out.append(states.CompoundThermodynamicState(states.ThermodynamicState(asys, T), [a]))
    return out


def run(name, sampler, n_iter, warm=1):
    sampler.run(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sampler.run(n_iter)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n_iter
    print(json.dumps(dict(config=name, iterations_per_s=1.0 / dt, ms_per_iteration=1e3 * dt, replicas=sampler.n_replicas,
                          states=sampler.n_states, timing={k: (v if isinstance(v, str) else float(v)) for k, v in sampler._timing_data.items()})), flush=True)


def main():
    which = sys.argv[1:] or ['2', '4', '5', '5h']
    def move(dt_fs, split):
        return mcmc.LangevinSplittingDynamicsMove(timestep=dt_fs * unit.femtosecond, collision_rate=1.0 / unit.picosecond,
                                                  n_steps=500, reassign_velocities=True, splitting=split)
    if '2' in which:
        lj = testsystems.LennardJonesFluid(nparticles=512)
        ths = alchemical_states(lj.system, range(10), np.ones(16), np.linspace(1.0, 0.0, 16))
        s = ReplicaExchangeSampler(mcmc_moves=move(1.0, 'V R O R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(ths, [states.SamplerState(lj.positions, box_vectors=lj.system.getDefaultPeriodicBoxVectors())])
        run('2: LennardJonesFluid(512), 16 lambda_sterics states, BAOAB 1 fs x 500', s, 5)
    if '4' in which:
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        ths = alchemical_states(hg.system, range(126, 156), lam_e, lam_s)
        # one GPU's share of the 64-replica ensemble: 8 replicas, all 64 states in u_kl (R != K => no swap-all; SAMS jump)
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4 (1-GPU share): HostGuestExplicit, 8 replicas x 64 alchemical states, g-BAOAB 2 fs x 500', s, 3)
    if '4mc' in which:
        # config 4's share with YANK's move set for binding free energies: displacement and rotation of the guest (atoms 126 .. 155), then
        # the dynamics; once with the proposals on the host, once on the device (mcmc.MetropolizedMove proposal=, csrc/mc_moves.hip)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        ths = alchemical_states(hg.system, range(126, 156), lam_e, lam_s)
        guest = list(range(126, 156))
        for proposal in ('host', 'device'):
            seq = mcmc.SequenceMove([mcmc.MCDisplacementMove(displacement_sigma=0.1 * unit.nanometer, atom_subset=guest, proposal=proposal),
                                     mcmc.MCRotationMove(atom_subset=guest, proposal=proposal), move(2.0, 'V R R O R R V')])
            s = SAMSSampler(mcmc_moves=seq, number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
            ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
            s.create(ths, [ss] * 8)
            run("4mc (1-GPU share, proposal='%s'): HostGuestExplicit, 8 replicas x 64 alchemical states, guest displacement + rotation, "
                'g-BAOAB 2 fs x 500' % proposal, s, 3)
    if 'wca' in which:
        # a System whose only pair force is a CustomNonbondedForce (custom_expr.py kind 6, csrc/custom_nonbonded.hip): 24-replica parallel
        # tempering of testsystems.WCAFluid (216 particles, no NonbondedForce)
        wca = testsystems.WCAFluid()
        s = ParallelTemperingSampler(mcmc_moves=move(2.0, 'V R O R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(wca.positions, box_vectors=wca.system.getDefaultPeriodicBoxVectors())
        s.create(states.ThermodynamicState(wca.system, 120.0 * unit.kelvin), [ss], storage=None, min_temperature=120.0 * unit.kelvin,
                 max_temperature=240.0 * unit.kelvin, n_temperatures=24)
        run('wca: WCAFluid(216), 24 temperatures 120 - 240 K, BAOAB 2 fs x 500', s, 5)
    if 'mw' in which:
        # monatomic water: a CustomNonbondedForce and a CustomManyParticleForce (custom_expr.py kind 11, csrc/custom_manyparticle.hip) are
        # the only forces: 24-replica parallel tempering of testsystems.StillingerWeberFluid (512 particles)
        mw = testsystems.StillingerWeberFluid(nparticles=512)
        s = ParallelTemperingSampler(mcmc_moves=move(5.0, 'V R O R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(mw.positions, box_vectors=mw.system.getDefaultPeriodicBoxVectors())
        s.create(states.ThermodynamicState(mw.system, 250.0 * unit.kelvin), [ss], storage=None, min_temperature=250.0 * unit.kelvin,
                 max_temperature=320.0 * unit.kelvin, n_temperatures=24)
        run('mw: StillingerWeberFluid(512, mW), 24 temperatures 250 - 320 K, BAOAB 5 fs x 500', s, 5)
    if 'hct' in which:
        # implicit-solvent parallel tempering with a CustomGBForce on the general path (custom_gb.compile_custom_gb, csrc/custom_gb.hip):
        # 24 temperatures of testsystems.AlanineDipeptideImplicit(implicitSolvent='HCT'); 'obc2' runs the same on csrc/gbsa.hip
        al = testsystems.AlanineDipeptideImplicit(implicitSolvent='HCT')
        s = ParallelTemperingSampler(mcmc_moves=move(2.0, 'V R O R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(states.ThermodynamicState(al.system, 300.0 * unit.kelvin), [states.SamplerState(al.positions)], storage=None,
                 min_temperature=300.0 * unit.kelvin, max_temperature=600.0 * unit.kelvin, n_temperatures=24)
        run('hct: AlanineDipeptideImplicit(HCT, CustomGBForce expressions), 24 temperatures 300 - 600 K, BAOAB 2 fs x 500', s, 5)
    if 'obc2' in which:
        al = testsystems.AlanineDipeptideImplicit()
        s = ParallelTemperingSampler(mcmc_moves=move(2.0, 'V R O R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(states.ThermodynamicState(al.system, 300.0 * unit.kelvin), [states.SamplerState(al.positions)], storage=None,
                 min_temperature=300.0 * unit.kelvin, max_temperature=600.0 * unit.kelvin, n_temperatures=24)
        run('obc2: AlanineDipeptideImplicit(OBC2, GBSAOBCForce), 24 temperatures 300 - 600 K, BAOAB 2 fs x 500', s, 5)
    if '4rs' in which:
        # config 4's share with a receptor-ligand restraint (forces.py, csrc/restraints.hip): a HarmonicRestraintForce between the CB7
        # heavy atoms and the B2 guest, K = 0.2 kcal/mol/A^2, lambda_restraints rising 0 -> 1 along the coupled half and 1 where the
        # guest is decoupled.  ('4r' is taken: the general-regions variant below.)
        from openmmtools_amd import forces

        class RestraintState(states.GlobalParameterState):
            lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        lam_r = np.concatenate([np.linspace(0.0, 1.0, 32), np.ones(32)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        heavy = [i for i in range(126) if hg.system.getParticleMass(i) > 1.5]
        asys.addForce(forces.HarmonicRestraintForce(0.2 * 4.184 * 100.0, heavy, list(range(126, 156))))
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le), RestraintState(lambda_restraints=lr)])
               for le, ls, lr in zip(lam_e, lam_s, lam_r)]
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4rs (1-GPU share, restrained): HostGuestExplicit + CB7/B2 HarmonicRestraintForce, 8 replicas x 64 states, g-BAOAB 2 fs x 500', s, 3)
    if '4cb' in which:
        # config 4's share with one custom bond force (custom_expr.py, csrc/custom_terms.hip): 30 bonds between the guest's atoms and CB7
        # heavy atoms, K = 0.2 kcal/mol/A^2, the global lambda_bonds rising 0 -> 1 along the coupled half and 1 where the guest is decoupled
        from openmmtools_amd.system import CustomBondForce

        class BondState(states.GlobalParameterState):
            lambda_bonds = states.GlobalParameterState.GlobalParameter('lambda_bonds', standard_value=1.0)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        lam_b = np.concatenate([np.linspace(0.0, 1.0, 32), np.ones(32)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        heavy = [i for i in range(126) if hg.system.getParticleMass(i) > 1.5]
        f = CustomBondForce('lambda_bonds*0.5*K*r^2')
        f.addGlobalParameter('lambda_bonds', 1.0)
        f.addPerBondParameter('K')
        for k, g in enumerate(range(126, 156)):
            f.addBond(heavy[(3 * k) % len(heavy)], g, [0.2 * 4.184 * 100.0 / 30.0])
        asys.addForce(f)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le), BondState(lambda_bonds=lb)])
               for le, ls, lb in zip(lam_e, lam_s, lam_b)]
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4cb (1-GPU share, custom bond force): HostGuestExplicit + a 30-bond CustomBondForce, 8 replicas x 64 states, g-BAOAB 2 fs x 500', s, 3)
    if '4bo' in which:
        # config 4's share with one orientational (Boresch) restraint (custom_expr.py, csrc/custom_compound.hip): a six-particle
        # CustomCompoundBondForce on three CB7 and three guest heavy atoms, the reference values the starting geometry's, the global
        # lambda_restraints rising 0 -> 1 along the coupled half and 1 where the guest is decoupled
        from openmmtools_amd.system import CustomCompoundBondForce

        class RestraintState(states.GlobalParameterState):
            lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        lam_r = np.concatenate([np.linspace(0.0, 1.0, 32), np.ones(32)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        heavy = [i for i in range(126) if hg.system.getParticleMass(i) > 1.5]
        guest = [i for i in range(126, 156) if hg.system.getParticleMass(i) > 1.5]
        atoms = [heavy[2 * len(heavy) // 3], heavy[len(heavy) // 3], heavy[0], guest[0], guest[len(guest) // 2], guest[-1]]
        f = CustomCompoundBondForce(6, 'lambda_restraints*E; E = (K_r/2)*(distance(p3,p4)-r_aA0)^2 + (K_thetaA/2)*(angle(p2,p3,p4)-theta_A0)^2 '
                                       '+ (K_thetaB/2)*(angle(p3,p4,p5)-theta_B0)^2 + (K_phiA/2)*dphi_A^2 + (K_phiB/2)*dphi_B^2 + (K_phiC/2)*dphi_C^2; '
                                       'dphi_A = dA - floor(dA/(2*pi)+0.5)*(2*pi); dA = dihedral(p1,p2,p3,p4)-phi_A0; '
                                       'dphi_B = dB - floor(dB/(2*pi)+0.5)*(2*pi); dB = dihedral(p2,p3,p4,p5)-phi_B0; '
                                       'dphi_C = dC - floor(dC/(2*pi)+0.5)*(2*pi); dC = dihedral(p3,p4,p5,p6)-phi_C0; pi = 3.1415926535897932385')
        f.addGlobalParameter('lambda_restraints', 1.0)
        x = np.asarray(hg.positions, dtype=np.float64)[atoms]

        def angle(i, j, k):
            u, v = x[i] - x[j], x[k] - x[j]
            return float(np.arccos(np.dot(u, v) / np.sqrt(np.dot(u, u) * np.dot(v, v))))

        def dihedral(i, j, k, l):
            b1, b2, b3 = x[j] - x[i], x[k] - x[j], x[l] - x[k]
            m, n = np.cross(b1, b2), np.cross(b2, b3)
            return float(np.arctan2(np.linalg.norm(b2) * np.dot(b1, n), np.dot(m, n)))
        reference = dict(r_aA0=float(np.linalg.norm(x[3] - x[2])), theta_A0=angle(1, 2, 3), theta_B0=angle(2, 3, 4), phi_A0=dihedral(0, 1, 2, 3),
                         phi_B0=dihedral(1, 2, 3, 4), phi_C0=dihedral(2, 3, 4, 5))
        springs = dict(K_r=20.0 * 4.184 * 100.0, K_thetaA=20.0 * 4.184, K_thetaB=20.0 * 4.184, K_phiA=20.0 * 4.184, K_phiB=20.0 * 4.184, K_phiC=20.0 * 4.184)
        values = dict(reference, **springs)
        for name in values:
            f.addPerBondParameter(name)
        f.addBond(atoms, list(values.values()))
        asys.addForce(f)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le), RestraintState(lambda_restraints=lr)])
               for le, ls, lr in zip(lam_e, lam_s, lam_r)]
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4bo (1-GPU share, Boresch restraint): HostGuestExplicit + one six-particle CustomCompoundBondForce, 8 replicas x 64 states, '
            'g-BAOAB 2 fs x 500', s, 3)
    for tag in ('4c1', '4cc'):
        if tag not in which:
            continue
        # config 4's share with one centroid bond (custom_expr.py, csrc/custom_centroid.hip): '4c1' between two single-atom groups (a CB7
        # and a guest heavy atom), '4cc' between the guest and ALL host atoms (30 and 126 atoms, mass weights); a quartic
        # wall on the centroid distance, its global lambda_com rising 0 -> 1 along the coupled half and 1 where the guest is decoupled.
        # After the timed iterations one more runs with the engine's profile on for the three launches of the feature.
        from openmmtools_amd.system import CustomCentroidBondForce

        class ComState(states.GlobalParameterState):
            lambda_com = states.GlobalParameterState.GlobalParameter('lambda_com', standard_value=1.0)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        lam_c = np.concatenate([np.linspace(0.0, 1.0, 32), np.ones(32)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        f = CustomCentroidBondForce(2, 'lambda_com*K*max(0, distance(g1,g2)-r0)^4')
        f.addGlobalParameter('lambda_com', 1.0)
        f.addPerBondParameter('K'); f.addPerBondParameter('r0')
        if tag == '4c1':
            heavy = [i for i in range(126) if hg.system.getParticleMass(i) > 1.5]
            guest = [i for i in range(126, 156) if hg.system.getParticleMass(i) > 1.5]
            f.addGroup([heavy[0]]); f.addGroup([guest[0]])
        else:
            f.addGroup(list(range(0, 126))); f.addGroup(list(range(126, 156)))
        f.addBond([0, 1], [500.0, 0.0])
        f.setUsesPeriodicBoundaryConditions(True)
        asys.addForce(f)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le), ComState(lambda_com=lc)])
               for le, ls, lc in zip(lam_e, lam_s, lam_c)]
        engine = HipEngine()
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=engine, seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('%s (1-GPU share, centroid bond of groups of %d and %d atoms): HostGuestExplicit + one CustomCentroidBondForce, 8 replicas x 64 '
            'states, g-BAOAB 2 fs x 500' % (tag, len(f.getGroupParameters(0)[0]), len(f.getGroupParameters(1)[0])), s, 3)
        engine.profile_enable(1, 'custom_centroid')
        engine.profile_reset()
        s.run(1)
        torch.cuda.synchronize()
        out = {}
        for name in ('custom_centroid_sum', 'custom_centroid_bonds', 'custom_centroid_spread'):
            n, ms = engine.profile_get(name)
            out[name] = dict(launches_timed=n, us_per_launch=1e3 * ms / max(n, 1))
        engine.profile_enable(0)
        print(json.dumps(dict(config=tag, profile=out)), flush=True)
    if '4rm' in which:
        # config 4's share with one RMSD restraint (custom_expr.py kind 7, csrc/custom_cv.hip): a harmonic CustomCVForce on the RMSD of
        # the 126 atoms of CB7 from the starting geometry, its spring constant k_rmsd rising 0 -> 2000 kJ/mol/nm^2 along the coupled half.
        # 126 atoms because RMSDForce takes no minimum images: CB7 is the largest molecule of the System, and a variable that spans
        # molecules is refused.  After the timed iterations one more runs with the engine's profile on for the three launches.
        from openmmtools_amd.system import CustomCVForce, RMSDForce

        class RmsdState(states.GlobalParameterState):
            k_rmsd = states.GlobalParameterState.GlobalParameter('k_rmsd', standard_value=1.0)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        k_r = np.concatenate([np.linspace(0.0, 2000.0, 32), np.full(32, 2000.0)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        f = CustomCVForce('0.5*k_rmsd*v^2')
        f.addGlobalParameter('k_rmsd', 2000.0)
        f.addCollectiveVariable('v', RMSDForce(hg.positions, list(range(0, 126))))
        asys.addForce(f)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le), RmsdState(k_rmsd=k)])
               for le, ls, k in zip(lam_e, lam_s, k_r)]
        engine = HipEngine()
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=engine, seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4rm (1-GPU share, RMSD restraint on the 126 atoms of CB7): HostGuestExplicit + one CustomCVForce, 8 replicas x 64 states, '
            'g-BAOAB 2 fs x 500', s, 3)
        engine.profile_enable(1, 'custom_cv')
        engine.profile_reset()
        s.run(1)
        torch.cuda.synchronize()
        out = {}
        for name in ('custom_cv_superpose', 'custom_cv_expression', 'custom_cv_spread'):
            n, ms = engine.profile_get(name)
            out[name] = dict(launches_timed=n, us_per_launch=1e3 * ms / max(n, 1))
        engine.profile_enable(0)
        print(json.dumps(dict(config='4rm', profile=out)), flush=True)
    if '4cm' in which:
        # config 4's share with a CMAPTorsionForce (custom_expr.py kind 8, csrc/cmap.hip): CB7 is no peptide, so the torsion pairs are
        # synthetic phi / psi-like quadruples of the host -- every run of five atoms along a bonded path, (a, b, c, d) and (b, c, d, e), on
        # two 24 x 24 maps.  After the timed iterations one more runs with the engine's profile on for the custom-force launches.
        from openmmtools_amd.system import CMAPTorsionForce, HarmonicBondForce
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156)))
        bonded = {}
        for f in hg.system.getForces():
            if isinstance(f, HarmonicBondForce):
                for k in range(f.getNumBonds()):
                    i, j = f.getBondParameters(k)[:2]
                    if i < 126 and j < 126:
                        bonded.setdefault(i, []).append(j); bonded.setdefault(j, []).append(i)
        paths = set()
        for a in sorted(bonded):
            for b in bonded[a]:
                for c in bonded[b]:
                    for d in bonded[c]:
                        for e in bonded[d]:
                            if len({a, b, c, d, e}) == 5 and a < e:
                                paths.add((a, b, c, d, e))
        paths = sorted(paths)[::4]
        angle = 2.0 * np.pi * np.arange(24) / 24
        cmap = CMAPTorsionForce()
        for k in range(2):
            cmap.addMap(24, (2.0 * np.cos(angle[None, :] + k) + 1.5 * np.sin(2.0 * angle[:, None]) + np.cos(angle[None, :] - angle[:, None])).reshape(-1))
        for t, (a, b, c, d, e) in enumerate(paths):
            cmap.addTorsion(t % 2, a, b, c, d, b, c, d, e)
        cmap.setUsesPeriodicBoundaryConditions(True)
        asys.addForce(cmap)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(lambda_sterics=ls, lambda_electrostatics=le)])
               for le, ls in zip(lam_e, lam_s)]
        engine = HipEngine()
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=engine, seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4cm (1-GPU share, %d CMAP torsion pairs on CB7): HostGuestExplicit + one CMAPTorsionForce, 8 replicas x 64 states, '
            'g-BAOAB 2 fs x 500' % len(paths), s, 3)
        engine.profile_enable(1, 'custom_terms')
        engine.profile_reset()
        s.run(1)
        n, ms = engine.profile_get('custom_terms')
        engine.profile_enable(0)
        print(json.dumps(dict(config='4cm', profile=dict(custom_terms=dict(launches_timed=n, us_per_launch=1e3 * ms / max(n, 1))))), flush=True)
    if '4cr' in which:
        # config 4's share with EVERY harmonic bond, harmonic angle and periodic torsion of the System moved to custom forces with the
        # same formulas (custom_expr.py): what the expression machine costs at a force field's size, against the built-in listed terms of '4'
        from openmmtools_amd.system import (CustomBondForce, CustomAngleForce, CustomTorsionForce, HarmonicBondForce, HarmonicAngleForce,
                                            PeriodicTorsionForce)
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        b = CustomBondForce('0.5*k*(r-r0)^2'); b.addPerBondParameter('r0'); b.addPerBondParameter('k')
        a = CustomAngleForce('0.5*k*(theta-theta0)^2'); a.addPerAngleParameter('theta0'); a.addPerAngleParameter('k')
        t = CustomTorsionForce('k*(1+cos(n*theta-phase))')
        for name in ('n', 'phase', 'k'):
            t.addPerTorsionParameter(name)
        for f in hg.system.getForces():
            if isinstance(f, HarmonicBondForce):
                for q in f.bonds: b.addBond(q[0], q[1], q[2:])
            elif isinstance(f, HarmonicAngleForce):
                for q in f.angles: a.addAngle(q[0], q[1], q[2], q[3:])
            elif isinstance(f, PeriodicTorsionForce):
                for q in f.torsions: t.addTorsion(q[0], q[1], q[2], q[3], q[4:])
        hg.system.forces = [f for f in hg.system.forces if not isinstance(f, (HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce))]
        for f in (b, a, t):
            hg.system.addForce(f)
        ths = alchemical_states(hg.system, range(126, 156), lam_e, lam_s)
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('4cr (1-GPU share, %d custom bonds + %d custom angles + %d custom torsions instead of the built-in ones): HostGuestExplicit, '
            '8 replicas x 64 states, g-BAOAB 2 fs x 500' % (b.getNumBonds(), a.getNumAngles(), t.getNumTorsions()), s, 3)
    for tag, kw in (('4r', dict()), ('4d', dict(alchemical_pme_treatment='direct-space'))):
        if tag not in which:
            continue
        # config 4's share on the GENERAL alchemical path (csrc/alch_regions.hip): the guest and the reference's second test region
        # (atoms 156-159, tests/test_alchemy.py:2203-2208) as two named regions, both on config 4's ladder; '4r': the exact PME treatment
        # (the regions' scaled charges inside the Ewald sum, u_kl from six energy passes), '4d': 'direct-space' soft-core electrostatics
        hg = testsystems.HostGuestExplicit()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 32), np.zeros(32)])
        lam_s = np.concatenate([np.ones(32), np.linspace(1.0, 0.0, 32)])
        regions = [alchemy.AlchemicalRegion(alchemical_atoms=range(126, 156), name='zero'), alchemy.AlchemicalRegion(alchemical_atoms=range(156, 160), name='one')]
        asys = alchemy.AbsoluteAlchemicalFactory(**kw).create_alchemical_system(hg.system, regions)
        ths = [states.CompoundThermodynamicState(states.ThermodynamicState(asys, 300.0),
                                                 [states.AlchemicalState(parameters_name_suffix='zero', lambda_sterics=ls, lambda_electrostatics=le),
                                                  states.AlchemicalState(parameters_name_suffix='one', lambda_sterics=ls, lambda_electrostatics=le)])
               for le, ls in zip(lam_e, lam_s)]
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 8)
        run('%s (1-GPU share, general alchemical regions, %s): HostGuestExplicit, 8 replicas x 64 states of two named regions, g-BAOAB 2 fs x 500'
            % (tag, kw.get('alchemical_pme_treatment', 'exact PME')), s, 3)
    for tag, cls in (('v', 'AlanineDipeptideVacuum'), ('g', 'AlanineDipeptideImplicit'), ('hv', 'HostGuestVacuum')):
        if tag not in which:
            continue
        # the reference's small NoCutoff test systems (csrc/nocutoff.hip, csrc/gbsa.hip): 24 temperatures, the headline's protocol
        t = getattr(testsystems, cls)()
        nt = int(os.environ.get('REMD_BENCH_NT', '24'))           # (swap-all timings at other ensemble sizes: profiles/r06_44)
        ths = [states.ThermodynamicState(t.system, T) for T in np.geomspace(300.0, 600.0, nt)]
        s = ReplicaExchangeSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(ths, [states.SamplerState(t.positions)])
        run('%s: %s (%d atoms, NoCutoff), %d temperatures, swap-all, g-BAOAB 2 fs x 500' % (tag, cls, t.system.getNumParticles(), nt), s, 5)
    for tag, model in (('w3', 'tip3p'), ('w4', 'tip4pew')):
        if tag not in which:
            continue
        # a water box of 522 molecules (testsystems.WaterBox at its default 2.5 nm edge) as three-site TIP3P and as four-site TIP4P-Ew,
        # whose charge site is a virtual site (csrc/virtual_sites.hip): the same molecule count, 24 temperatures, the headline's protocol;
        # the difference per iteration is what the sites cost (one more particle per water, the two launches per force evaluation, the
        # join by a launch instead of in the chain).  The lattice start is relaxed by FIRE first.
        wb = testsystems.WaterBox(model=model)
        ths = [states.ThermodynamicState(wb.system, T) for T in np.geomspace(300.0, 400.0, 24)]
        s = ReplicaExchangeSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(ths, [states.SamplerState(wb.positions, box_vectors=wb.system.getDefaultPeriodicBoxVectors())])
        s.minimize(max_iterations=200)
        run('%s: WaterBox(%s), %d waters = %d particles, 24 temperatures, swap-all, g-BAOAB 2 fs x 500'
            % (tag, model, wb.n_waters, wb.system.getNumParticles()), s, 3)
    if 'n' in which:
        # the headline ensemble at constant pressure (NPT states: Monte Carlo barostat every 25 steps inside the propagation)
        al = testsystems.AlanineDipeptideExplicit()
        ths = [states.ThermodynamicState(al.system, T, pressure=1.0 * unit.atmosphere) for T in np.geomspace(300.0, 600.0, 24)]
        s = ReplicaExchangeSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        s.create(ths, [states.SamplerState(al.positions, box_vectors=al.system.getDefaultPeriodicBoxVectors())])
        run('n: AlanineDipeptideExplicit, 24 temperatures at 1 atm (Monte Carlo barostat every 25 steps), swap-all, g-BAOAB 2 fs x 500', s, 5)
    if '5' in which:
        dh = testsystems.DHFRExplicit()
        T = np.geomspace(300.0, 400.0, 128)
        ths = [states.ThermodynamicState(dh.system, t) for t in T]
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(dh.positions, box_vectors=dh.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 16)
        run('5 (1-GPU share): DHFRExplicit 23558 atoms, 16 replicas x 128 temperature states, SAMS global jump, g-BAOAB 2 fs x 500', s, 2)
    if '5h' in which:
        # the same share with north_star's wording: 128 HAMILTONIAN replicas = an alchemical ladder (ten solvent molecules decoupled)
        dh = testsystems.DHFRExplicit()
        n = dh.system.getNumParticles()
        lam_e = np.concatenate([np.linspace(1.0, 0.0, 64), np.zeros(64)])
        lam_s = np.concatenate([np.ones(64), np.linspace(1.0, 0.0, 64)])
        ths = alchemical_states(dh.system, range(n - 30, n), lam_e, lam_s)
        s = SAMSSampler(mcmc_moves=move(2.0, 'V R R O R R V'), number_of_iterations=10 ** 9, engine=HipEngine(), seed=1)
        ss = states.SamplerState(dh.positions, box_vectors=dh.system.getDefaultPeriodicBoxVectors())
        s.create(ths, [ss] * 16)
        run('5h (1-GPU share): DHFRExplicit 23558 atoms, 16 replicas x 128 alchemical states, SAMS global jump, g-BAOAB 2 fs x 500', s, 2)


if __name__ == '__main__':
    main()
