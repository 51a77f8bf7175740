"""ctypes binding of libremd_hip.so (the C ABI in include/remd_hip.h) and the HipEngine wrapper.

This is the product path.  There is deliberately NO CPU fallback: if the shared library is
missing, or no gfx950 device is visible, construction raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libremd_hip.so')

MIX_SCHEMES = {None: 0, 'none': 0, 'swap-all': 1, 'swap-neighbors': 2, 'sams-global-jump': 3}

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)


class RemdSystemDesc(C.Structure):
    _fields_ = [
        ('n_atoms', C.c_int32), ('mass', c_double_p),
        ('n_ext', C.c_int32), ('ext_atoms', c_int32_p),
        ('ext_K', C.c_double), ('ext_x0', C.c_double), ('ext_U0', C.c_double),
        ('n_bonds', C.c_int32), ('bond_atoms', c_int32_p), ('bond_params', c_double_p),
        ('n_angles', C.c_int32), ('angle_atoms', c_int32_p), ('angle_params', c_double_p),
        ('n_torsions', C.c_int32), ('torsion_atoms', c_int32_p), ('torsion_params', c_double_p),
        ('nb_method', C.c_int32), ('cutoff', C.c_double), ('switch_distance', C.c_double),
        ('rf_dielectric', C.c_double), ('ewald_alpha', C.c_double), ('pme_grid', C.c_int32 * 3),
        ('use_dispersion_correction', C.c_int32),
        ('charge', c_double_p), ('sigma', c_double_p), ('epsilon', c_double_p),
        ('n_exceptions', C.c_int32), ('exception_atoms', c_int32_p), ('exception_params', c_double_p),
        ('n_settle', C.c_int32), ('settle_atoms', c_int32_p), ('settle_dOH', C.c_double), ('settle_dHH', C.c_double),
        ('n_shake', C.c_int32), ('shake_atoms', c_int32_p), ('shake_dist', c_double_p),
        ('cmm_frequency', C.c_int32),
        ('n_alch', C.c_int32), ('alch_atoms', c_int32_p),
        ('softcore_alpha', C.c_double), ('softcore_a', C.c_double), ('softcore_b', C.c_double), ('softcore_c', C.c_double),
    ]


class RemdAlchRegionsDesc(C.Structure):
    """remd_alch_regions_desc of include/remd_hip.h (general alchemical regions)."""
    _fields_ = [
        ('n_atoms', C.c_int32), ('n_regions', C.c_int32), ('region_of_atom', c_int32_p), ('softcore', c_double_p), ('annihilate', c_int32_p),
        ('n_interactions', C.c_int32), ('interactions', c_int32_p),
        ('charge', c_double_p), ('sigma', c_double_p), ('epsilon', c_double_p),
        ('n_exceptions', C.c_int32), ('exception_atoms', c_int32_p), ('exception_params', c_double_p),
        ('electrostatics', C.c_int32),
        ('elec_alpha', C.c_double), ('elec_krf', C.c_double), ('elec_crf', C.c_double), ('elec_switch_distance', C.c_double),
        ('exact_pme', C.c_int32),
        ('n_bonds', C.c_int32), ('bond_atoms', c_int32_p), ('bond_params', c_double_p), ('bond_region', c_int32_p),
        ('n_angles', C.c_int32), ('angle_atoms', c_int32_p), ('angle_params', c_double_p), ('angle_region', c_int32_p),
        ('n_torsions', C.c_int32), ('torsion_atoms', c_int32_p), ('torsion_params', c_double_p), ('torsion_region', c_int32_p),
        ('consistent_exceptions', C.c_int32),
    ]


class RemdGbsaDesc(C.Structure):
    """remd_gbsa_desc of include/remd_hip.h (GBSA OBC2 + ACE of a NoCutoff system)."""
    _fields_ = [('n_atoms', C.c_int32), ('charge', c_double_p), ('radius', c_double_p), ('scale', c_double_p), ('alchemical', c_int32_p),
                ('solute_dielectric', C.c_double), ('solvent_dielectric', C.c_double), ('surface_area', C.c_int32)]


class RemdRestraintDesc(C.Structure):
    """remd_restraint_desc of include/remd_hip_restraints.h (receptor-ligand restraints, forces.py)."""
    _fields_ = [('kind', C.c_int32), ('K', C.c_double), ('r0', C.c_double),
                ('n1', C.c_int32), ('atoms1', c_int32_p), ('weights1', c_double_p),
                ('n2', C.c_int32), ('atoms2', c_int32_p), ('weights2', c_double_p),
                ('periodic', C.c_int32), ('force_group', C.c_int32)]


class RemdCustomForceDesc(C.Structure):
    """remd_custom_force_desc of include/remd_hip_custom.h (custom bond / angle / torsion / external / compound-bond / centroid-bond
    forces, custom_expr.py)."""
    _fields_ = [('kind', C.c_int32), ('n_terms', C.c_int32), ('atoms', c_int32_p), ('n_params', C.c_int32), ('params', c_double_p),
                ('n_program', C.c_int32), ('program', c_int32_p), ('n_consts', C.c_int32), ('consts', c_double_p),
                ('stack_depth', C.c_int32), ('n_globals', C.c_int32), ('global_defaults', c_double_p),
                ('periodic', C.c_int32), ('force_group', C.c_int32), ('n_particles', C.c_int32),
                ('n_groups', C.c_int32), ('group_offsets', c_int32_p), ('group_atoms', c_int32_p), ('group_weights', c_double_p),
                ('nb_method', C.c_int32), ('cutoff', C.c_double), ('switch_distance', C.c_double), ('excl_offsets', c_int32_p),
                ('excl_atoms', c_int32_p), ('long_range_correction', C.c_int32),
                ('n_cvs', C.c_int32), ('cv_offsets', c_int32_p), ('cv_atoms', c_int32_p), ('cv_reference', c_double_p)]


class RemdCustomForceDescCMAP(RemdCustomForceDesc):
    """remd_custom_force_desc as remd_set_custom_terms takes it: the fields above, then those REMD_CUSTOM_CMAP appended at the end of
    the struct (a ctypes subclass lays its own fields out behind the base's, as C does behind a pointer member)"""
    _fields_ = [('map_index', c_int32_p), ('n_maps', C.c_int32), ('map_offsets', c_int32_p)]


class RemdCustomForceDescHbond(RemdCustomForceDescCMAP):
    """the same, then the fields of REMD_CUSTOM_HBOND behind those of REMD_CUSTOM_CMAP: the whole remd_custom_force_desc"""
    _fields_ = [('hb_n_donors', C.c_int32), ('hb_n_acceptors', C.c_int32), ('hb_donor_atoms', c_int32_p), ('hb_acceptor_atoms', c_int32_p),
                ('hb_n_donor_params', C.c_int32), ('hb_donor_params', c_double_p), ('hb_n_acceptor_params', C.c_int32),
                ('hb_acceptor_params', c_double_p), ('hb_excl_offsets', c_int32_p), ('hb_excl_acceptors', c_int32_p),
                ('hb_particle_mask', C.c_int32)]


class RemdCustomForceDescManyParticle(RemdCustomForceDescHbond):
    """the same, then the fields of REMD_CUSTOM_MANYPARTICLE behind those of REMD_CUSTOM_HBOND: the whole remd_custom_force_desc"""
    _fields_ = [('mp_types', c_int32_p), ('mp_permutation_mode', C.c_int32), ('mp_filter', C.c_uint32 * 3), ('mp_particle_mask', C.c_int32)]


class RemdCustomForceDescGB(RemdCustomForceDescManyParticle):
    """the same, then the fields of REMD_CUSTOM_GB behind those of REMD_CUSTOM_MANYPARTICLE: the whole remd_custom_force_desc"""
    _fields_ = [('gb_stages', c_int32_p), ('gb_n_values', C.c_int32), ('gb_n_stages', C.c_int32)]    # (the pointer first, as in C)


class RemdFrameCvTables(C.Structure):
    """remd_frame_cv_tables of include/remd_hip_frame_cvs.h (the collective variables of a call as CSR tables)."""
    _fields_ = [('n_cv', C.c_int32), ('kind', c_int32_p), ('periodic', c_int32_p), ('cv_groups', c_int32_p), ('group_off', c_int32_p),
                ('atoms', c_int32_p), ('weights', c_double_p), ('reference', c_double_p)]


class RemdGbModelDesc(C.Structure):
    """remd_gb_model_desc of include/remd_hip_gb.h (the constants and the cutoff of an OBC-family implicit-solvent model)."""
    _fields_ = [('offset', C.c_double), ('alpha', C.c_double), ('beta', C.c_double), ('gamma', C.c_double), ('ke', C.c_double),
                ('surface', C.c_double), ('probe', C.c_double), ('method', C.c_int32), ('cutoff', C.c_double)]


# the GPU-only extension of include/remd_hip_restraints.h: bound where the loaded library exports it (the CPU port of the ABI does not)
RESTRAINT_EXPORTS = ['remd_set_restraints', 'remd_set_restraint_lambdas', 'remd_get_restraint_energies']
# the analysis pass over stored frames of the same header (no handle: a device), bound the same way
RESTRAINT_FRAMES_EXPORTS = ['remd_restraint_frames', 'remd_restraint_frames_last_ms']
# the GPU-only extension of include/remd_hip_frame_cvs.h (collective variables of stored frames; no handle: a device), bound the same way
FRAME_CVS_EXPORTS = ['remd_frame_cvs']
# the GPU-only extension of include/remd_hip_custom.h (custom bond / angle / torsion / external forces), bound the same way
CUSTOM_EXPORTS = ['remd_set_custom_terms', 'remd_set_custom_globals', 'remd_set_custom_lrc', 'remd_get_custom_energies']
# the collective-variable forces of the same header (REMD_CUSTOM_CV): a library built before them lacks the entry point
CUSTOM_CV_EXPORTS = ['remd_get_custom_cv_values']
# the energy parameter derivatives of the same header: a library built before them lacks the entry points
CUSTOM_DERIVATIVE_EXPORTS = ['remd_set_custom_parameter_derivatives', 'remd_get_custom_parameter_derivatives']
# the same at every state's globals (thermodynamic integration): a library built before it lacks the entry point
CUSTOM_DERIVATIVE_STATES_EXPORTS = ['remd_get_custom_parameter_derivatives_at_states']
# the GPU-only extension of include/remd_hip_barostat.h (per-axis Monte Carlo barostats), bound the same way
BAROSTAT_AXIS_EXPORTS = ['remd_set_barostat_axes', 'remd_get_barostat_axis_stats']
BAROSTAT_ANISOTROPIC, BAROSTAT_MEMBRANE = 1, 2
# the GPU-only extension of include/remd_hip_mbar.h (the passes of the MBAR estimator), bound the same way
MBAR_EXPORTS = ['remd_mbar_create', 'remd_mbar_destroy', 'remd_mbar_log_denominator', 'remd_mbar_self_consistent', 'remd_mbar_newton_parts',
                'remd_mbar_gram', 'remd_mbar_log_weights', 'remd_mbar_chunks', 'remd_mbar_last_ms']
MBAR_MAX_STATES = 512
# the augmented Gram matrix of the same header (perturbed states and observables): a library built before it lacks the entry point
MBAR_AUGMENTED_EXPORTS = ['remd_mbar_augmented_gram']
# the bootstrap replicates of the same header (multiplicities drawn on the device, the batched weighted passes), bound the same way
MBAR_BOOTSTRAP_EXPORTS = ['remd_mbar_bootstrap_max_batch', 'remd_mbar_bootstrap_draw', 'remd_mbar_bootstrap_counts',
                          'remd_mbar_bootstrap_log_denominator', 'remd_mbar_bootstrap_self_consistent', 'remd_mbar_bootstrap_newton_parts',
                          'remd_mbar_bootstrap_rows']
# the free energy surfaces over binned samples of the same header (a bin index per sample), bound the same way
MBAR_PMF_EXPORTS = ['remd_mbar_pmf_chunk', 'remd_mbar_pmf', 'remd_mbar_bootstrap_pmf']
MBAR_PMF_MAX_BINS = 65536
# the GPU-only extension of include/remd_hip_timeseries.h (statistical inefficiencies of the suffixes of a timeseries), bound the same way
TIMESERIES_EXPORTS = ['remd_timeseries_create', 'remd_timeseries_destroy', 'remd_timeseries_inefficiency', 'remd_timeseries_chunks',
                      'remd_timeseries_last_ms']
TIMESERIES_MAX_BATCH = 64
# the GPU-only extension of include/remd_hip_energy_store.h (the stored energies and state indices of a run on the device), bound the same way
ENERGY_STORE_EXPORTS = ['remd_energy_store_create', 'remd_energy_store_destroy', 'remd_energy_store_effective_energy',
                        'remd_energy_store_gather_u_ln', 'remd_energy_store_transition_counts', 'remd_energy_store_chunks',
                        'remd_energy_store_last_ms', 'remd_series_inefficiency_multiple', 'remd_series_inefficiency_multiple_batched']
SERIES_MAX_BATCH = 64
# the GPU-only extension of include/remd_hip_vsites.h (virtual sites), bound the same way
VSITE_EXPORTS = ['remd_set_virtual_sites']


class RemdVsiteDesc(C.Structure):
    """remd_vsite_desc (include/remd_hip_vsites.h)."""
    _fields_ = [('kind', C.c_int32), ('site', C.c_int32), ('parent', C.c_int32 * 3), ('weight', C.c_double * 3)]


# the GPU-only extension of include/remd_hip_mcmoves.h (Metropolized rigid-body moves on the device), bound the same way
MC_MOVE_EXPORTS = ['remd_mc_rigid_moves']
MC_DISPLACEMENT, MC_ROTATION, MC_MAX_MOVES = 0, 1, 16


class RemdMcMoveDesc(C.Structure):
    """remd_mc_move_desc (include/remd_hip_mcmoves.h)."""
    _fields_ = [('kind', C.c_int32), ('n_atoms', C.c_int32), ('atoms', C.POINTER(C.c_int32)), ('sigma_nm', C.c_double),
                ('position', C.c_int32)]

EXPORTS = [
    'remd_create', 'remd_destroy', 'remd_last_error', 'remd_version', 'remd_set_system', 'remd_set_coulomb_cutoff', 'remd_set_reaction_field', 'remd_set_alchemical_options', 'remd_set_alchemical_regions',
    'remd_set_region_lambdas', 'remd_set_region_bonded_lambdas', 'remd_set_gbsa', 'remd_set_states',
    'remd_set_integrator', 'remd_set_replicas', 'remd_set_replica_ids', 'remd_copy_replicas', 'remd_set_labels', 'remd_seed', 'remd_propagate',
    'remd_compute_energies', 'remd_ukl_device_ptr', 'remd_mix', 'remd_mix_host', 'remd_get_replicas',
    'remd_get_forces', 'remd_get_group_forces', 'remd_propagate_many', 'remd_set_phases', 'remd_get_phases', 'remd_get_constraint_stats', 'remd_step', 'remd_sync', 'remd_last_timing', 'remd_profile_enable',
    'remd_profile_get', 'remd_profile_reset', 'remd_test_fft3d', 'remd_get_energy_components', 'remd_profile_filter',
    'remd_set_restart_attempts', 'remd_set_force_groups', 'remd_set_work_measurement', 'remd_get_work', 'remd_reset_work', 'remd_minimize', 'remd_set_barostat', 'remd_get_boxes', 'remd_get_barostat_stats',
    'remd_barostat_attempts',
    'remd_set_energy_const_volume', 'remd_roof_microbench', 'remd_roof_clock_ghz', 'remd_roof_pair_step', 'remd_test_coulomb_table',
    'remd_comm_unique_id', 'remd_comm_init', 'remd_comm_all_gather_energies', 'remd_comm_finalize',
]

_lib = None

# the split of the Ewald sum a HipEngine on the device asks the host classes for when nothing else is said (HipEngine.__init__):
# 'auto' = system.rebalanced_coulomb_cutoff.  Measured on the three PME systems of BASELINE.json (profiles/r04_a_ewald_split_sweep.txt,
# ms per 500 MD steps, reference -> auto): 24 x alanine dipeptide 104.5 -> 95.0, 8 x host-guest 99.7 -> 91.4, 16 x DHFR 836 -> 790.
DEFAULT_EWALD_SPLIT = os.environ.get('REMD_EWALD_SPLIT', 'auto')


def load_library(path=None):
    """dlopen libremd_hip.so and declare every prototype of include/remd_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH        # another build of the same ABI only by an explicit lib_path (tests, tools): no environment hook
    if not os.path.exists(path):
        raise RuntimeError('%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 + libhsa-runtime64 (used for the RCCL
    # all-gather), and a process that initialises the system ROCm runtime first leaves torch with "No HIP GPUs are
    # available".  Loading torch first makes libremd_hip.so's NEEDED libamdhip64.so.7 resolve to the already loaded copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.remd_create.argtypes = [C.POINTER(vp), C.c_int, vp]
    lib.remd_destroy.argtypes = [vp]
    lib.remd_last_error.argtypes = [vp]
    lib.remd_last_error.restype = C.c_char_p
    lib.remd_version.argtypes = []
    lib.remd_set_system.argtypes = [vp, C.POINTER(RemdSystemDesc)]
    lib.remd_set_coulomb_cutoff.argtypes = [vp, C.c_double]
    lib.remd_set_reaction_field.argtypes = [vp, C.c_int, C.c_double]
    lib.remd_set_alchemical_options.argtypes = [vp, C.c_int]
    lib.remd_set_alchemical_regions.argtypes = [vp, C.POINTER(RemdAlchRegionsDesc)]
    lib.remd_set_region_lambdas.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p]
    lib.remd_set_region_bonded_lambdas.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]
    lib.remd_set_gbsa.argtypes = [vp, C.POINTER(RemdGbsaDesc)]
    lib.remd_set_states.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.remd_set_integrator.argtypes = [vp, C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double]
    lib.remd_set_restart_attempts.argtypes = [vp, C.c_int]
    lib.remd_set_force_groups.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.remd_set_work_measurement.argtypes = [vp, C.c_int, C.c_int]
    lib.remd_get_work.argtypes = [vp, c_double_p, c_double_p, c_int64_p, c_int64_p]
    lib.remd_reset_work.argtypes = [vp]
    lib.remd_minimize.argtypes = [vp, C.c_double, C.c_int, c_int32_p, c_int32_p]
    lib.remd_set_barostat.argtypes = [vp, C.c_int, c_double_p, C.c_int]
    lib.remd_get_boxes.argtypes = [vp, c_double_p]
    lib.remd_set_energy_const_volume.argtypes = [vp, C.c_double]
    lib.remd_get_barostat_stats.argtypes = [vp, c_double_p, c_int64_p, c_int64_p]
    lib.remd_barostat_attempts.argtypes = [vp, C.c_int]
    lib.remd_set_replicas.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_int64_p]
    lib.remd_set_replica_ids.argtypes = [vp, c_int64_p]
    lib.remd_copy_replicas.argtypes = [vp, c_int32_p, vp, c_int32_p, C.c_int32, C.c_int32]
    lib.remd_set_labels.argtypes = [vp, c_int64_p]
    lib.remd_seed.argtypes = [vp, C.c_uint64]
    lib.remd_propagate.argtypes = [vp, C.c_int64, c_int32_p]
    lib.remd_compute_energies.argtypes = [vp, vp, c_double_p, c_double_p]
    lib.remd_ukl_device_ptr.argtypes = [vp, C.POINTER(vp)]
    lib.remd_mix.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, vp, C.c_int, c_int64_p, c_int64_p, c_int64_p,
                             c_double_p, c_double_p]
    lib.remd_mix_host.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, c_double_p, c_int64_p, c_int64_p,
                                  c_int64_p, c_double_p, c_double_p, C.c_int64]
    lib.remd_get_replicas.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.remd_get_forces.argtypes = [vp, c_double_p]
    lib.remd_get_group_forces.argtypes = [vp, C.c_uint32, c_double_p]
    lib.remd_propagate_many.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.POINTER(C.c_int32)]
    lib.remd_get_constraint_stats.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.remd_set_phases.argtypes = [vp, C.c_int32]
    lib.remd_get_phases.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.remd_step.argtypes = [vp, C.c_char_p, C.c_int64, C.c_int64, C.c_int]
    lib.remd_sync.argtypes = [vp]
    lib.remd_get_energy_components.argtypes = [vp, c_double_p]
    lib.remd_test_fft3d.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.remd_last_timing.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    lib.remd_profile_enable.argtypes = [vp, C.c_int]
    lib.remd_profile_get.argtypes = [vp, C.c_char_p, c_int64_p, c_double_p]
    lib.remd_profile_reset.argtypes = [vp]
    lib.remd_profile_filter.argtypes = [vp, C.c_char_p]
    lib.remd_roof_microbench.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    lib.remd_roof_clock_ghz.argtypes = [vp, c_double_p]
    lib.remd_roof_pair_step.argtypes = [vp, C.c_int, C.c_int, C.c_double, c_double_p, c_double_p]
    lib.remd_test_coulomb_table.argtypes = [C.c_double, C.c_double, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for name in EXPORTS:
        if name not in ('remd_last_error',):
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_set_restraints'):
        lib.remd_set_restraints.argtypes = [vp, C.POINTER(RemdRestraintDesc), C.c_int]
        lib.remd_set_restraint_lambdas.argtypes = [vp, c_double_p]
        lib.remd_get_restraint_energies.argtypes = [vp, c_double_p]
        for name in RESTRAINT_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_restraint_frames'):
        lib.remd_restraint_frames.argtypes = [C.c_int, C.POINTER(RemdRestraintDesc), C.c_int64, C.c_int, C.POINTER(C.c_float),
                                              C.POINTER(C.c_float), c_double_p, C.c_int64, c_double_p, c_double_p]
        lib.remd_restraint_frames_last_ms.argtypes = [c_double_p]
        for name in RESTRAINT_FRAMES_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_frame_cvs'):                    # include/remd_hip_frame_cvs.h (GPU-only, like the restraints)
        lib.remd_frame_cvs.argtypes = [C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(RemdFrameCvTables),
                                       C.c_int64, c_double_p, c_double_p]
        lib.remd_frame_cvs.restype = C.c_int
    if hasattr(lib, 'remd_set_custom_terms'):             # include/remd_hip_custom.h (GPU-only, like the restraints)
        lib.remd_set_custom_terms.argtypes = [vp, C.POINTER(RemdCustomForceDescGB), C.c_int]
        lib.remd_set_custom_globals.argtypes = [vp, c_double_p]
        lib.remd_set_custom_lrc.argtypes = [vp, c_double_p]
        lib.remd_get_custom_energies.argtypes = [vp, c_double_p]
        for name in CUSTOM_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_get_custom_cv_values'):
        lib.remd_get_custom_cv_values.argtypes = [vp, c_double_p]
    if hasattr(lib, 'remd_set_custom_parameter_derivatives'):
        lib.remd_set_custom_parameter_derivatives.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint32)]
        lib.remd_get_custom_parameter_derivatives.argtypes = [vp, c_double_p]
        for name in CUSTOM_DERIVATIVE_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_get_custom_parameter_derivatives_at_states'):
        lib.remd_get_custom_parameter_derivatives_at_states.argtypes = [vp, c_double_p]
        lib.remd_get_custom_parameter_derivatives_at_states.restype = C.c_int
        for name in CUSTOM_CV_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_set_barostat_axes'):            # include/remd_hip_barostat.h (GPU-only, like the restraints)
        lib.remd_set_barostat_axes.argtypes = [vp, C.c_int, c_double_p, c_double_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.remd_get_barostat_axis_stats.argtypes = [vp, c_double_p, c_int64_p, c_int64_p]
        for name in BAROSTAT_AXIS_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_set_gb_model'):                 # include/remd_hip_gb.h (GPU-only, like the restraints)
        lib.remd_set_gb_model.argtypes = [vp, C.POINTER(RemdGbModelDesc)]
        lib.remd_set_gb_model.restype = C.c_int
    if hasattr(lib, 'remd_set_virtual_sites'):            # include/remd_hip_vsites.h (GPU-only, like the restraints)
        lib.remd_set_virtual_sites.argtypes = [vp, C.POINTER(RemdVsiteDesc), C.c_int32]
        lib.remd_set_virtual_sites.restype = C.c_int
    if hasattr(lib, 'remd_mc_rigid_moves'):               # include/remd_hip_mcmoves.h (GPU-only, like the restraints)
        lib.remd_mc_rigid_moves.argtypes = [vp, C.POINTER(RemdMcMoveDesc), C.c_int32, C.c_int64, c_int32_p]
        lib.remd_mc_rigid_moves.restype = C.c_int
    if hasattr(lib, 'remd_mbar_create'):                  # include/remd_hip_mbar.h (GPU-only, like the restraints)
        lib.remd_mbar_create.argtypes = [C.c_int, C.c_int, C.c_int64, c_double_p, c_int64_p, C.POINTER(vp)]
        lib.remd_mbar_destroy.argtypes = [vp]
        lib.remd_mbar_log_denominator.argtypes = [vp, c_double_p, c_double_p, c_double_p]
        lib.remd_mbar_self_consistent.argtypes = [vp, c_double_p, c_double_p]
        lib.remd_mbar_newton_parts.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_double_p]
        lib.remd_mbar_gram.argtypes = [vp, c_double_p, C.c_int, c_double_p, c_double_p]
        lib.remd_mbar_log_weights.argtypes = [vp, c_double_p, c_double_p]
        lib.remd_mbar_chunks.argtypes = [vp, C.c_int, c_int64_p, c_int64_p, c_int64_p]
        lib.remd_mbar_last_ms.argtypes = [vp, c_double_p]
        for name in MBAR_EXPORTS:
            getattr(lib, name).restype = None if name == 'remd_mbar_destroy' else C.c_int
    if hasattr(lib, 'remd_mbar_augmented_gram'):
        lib.remd_mbar_augmented_gram.argtypes = [vp, c_double_p, C.c_int, c_double_p, C.c_int, c_double_p, c_int32_p, c_double_p, c_double_p,
                                                 c_double_p]
        lib.remd_mbar_augmented_gram.restype = C.c_int
    if hasattr(lib, 'remd_mbar_bootstrap_draw'):
        lib.remd_mbar_bootstrap_max_batch.argtypes = [vp, C.POINTER(C.c_int)]
        lib.remd_mbar_bootstrap_draw.argtypes = [vp, C.c_uint64, c_int32_p, C.c_int, C.c_int]
        lib.remd_mbar_bootstrap_counts.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
        lib.remd_mbar_bootstrap_log_denominator.argtypes = [vp, C.c_int, c_int32_p, c_double_p, c_double_p, c_double_p]
        lib.remd_mbar_bootstrap_self_consistent.argtypes = [vp, C.c_int, c_int32_p, c_double_p, c_double_p]
        lib.remd_mbar_bootstrap_newton_parts.argtypes = [vp, C.c_int, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p]
        lib.remd_mbar_bootstrap_rows.argtypes = [vp, C.c_int, c_int32_p, c_double_p, C.c_int, c_double_p, C.c_int, c_double_p, c_int32_p,
                                                 c_double_p, c_double_p]
        for name in MBAR_BOOTSTRAP_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_mbar_pmf'):
        lib.remd_mbar_pmf_chunk.argtypes = [vp, c_int64_p]
        lib.remd_mbar_pmf.argtypes = [vp, c_double_p, c_double_p, c_int32_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
        lib.remd_mbar_bootstrap_pmf.argtypes = [vp, C.c_int, c_int32_p, c_double_p, c_double_p, c_int32_p, C.c_int, c_double_p]
        for name in MBAR_PMF_EXPORTS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, 'remd_timeseries_create'):            # include/remd_hip_timeseries.h (GPU-only, like the restraints)
        lib.remd_timeseries_create.argtypes = [C.c_int, C.c_int64, c_double_p, C.POINTER(vp)]
        lib.remd_timeseries_destroy.argtypes = [vp]
        lib.remd_timeseries_inefficiency.argtypes = [vp, C.c_int32, c_int64_p, C.c_int, C.c_int, c_double_p, c_int32_p, c_int64_p]
        lib.remd_timeseries_chunks.argtypes = [vp, c_int64_p]
        lib.remd_timeseries_last_ms.argtypes = [vp, c_double_p]
        for name in TIMESERIES_EXPORTS:
            getattr(lib, name).restype = None if name == 'remd_timeseries_destroy' else C.c_int
    if hasattr(lib, 'remd_energy_store_create'):          # include/remd_hip_energy_store.h (GPU-only, like the restraints)
        lib.remd_energy_store_create.argtypes = [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_int32_p,
                                                 C.POINTER(vp)]
        lib.remd_energy_store_destroy.argtypes = [vp]
        lib.remd_energy_store_effective_energy.argtypes = [vp, c_double_p, c_double_p, c_double_p]
        lib.remd_energy_store_gather_u_ln.argtypes = [vp, C.c_int64, c_int64_p, c_double_p, c_int64_p]
        lib.remd_energy_store_transition_counts.argtypes = [vp, C.c_int64, C.c_int64, c_int64_p]
        lib.remd_energy_store_chunks.argtypes = [vp, c_int64_p, c_int64_p, c_int64_p, c_int32_p]
        lib.remd_energy_store_last_ms.argtypes = [vp, c_double_p]
        lib.remd_series_inefficiency_multiple.argtypes = [C.c_int, C.c_int32, C.c_int64, c_double_p, C.c_int, C.c_int, c_double_p, c_int32_p,
                                                          c_int64_p]
        lib.remd_series_inefficiency_multiple_batched.argtypes = [C.c_int, C.c_int32, C.c_int64, c_double_p, C.c_int, C.c_int, C.c_int32,
                                                                  c_double_p, c_int32_p, c_int64_p, c_double_p, c_int64_p]
        for name in ENERGY_STORE_EXPORTS:
            getattr(lib, name).restype = None if name == 'remd_energy_store_destroy' else C.c_int
    if path == LIB_PATH:
        _lib = lib
    return lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_int32_p)


def _lp(a):
    return None if a is None else a.ctypes.data_as(c_int64_p)


def build_desc(d):
    """Turn the dict from system.system_to_desc into a RemdSystemDesc (+ keep-alive list)."""
    keep = []

    def f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return _dp(a)

    def i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        keep.append(a)
        return _ip(a)

    s = RemdSystemDesc()
    s.n_atoms = int(d['n_atoms']); s.mass = f64(d['mass'])
    s.n_ext = int(d['n_ext']); s.ext_atoms = i32(d['ext_atoms'])
    s.ext_K, s.ext_x0, s.ext_U0 = float(d['ext_K']), float(d['ext_x0']), float(d['ext_U0'])
    s.n_bonds = len(d['bond_atoms']); s.bond_atoms = i32(d['bond_atoms']); s.bond_params = f64(d['bond_params'])
    s.n_angles = len(d['angle_atoms']); s.angle_atoms = i32(d['angle_atoms']); s.angle_params = f64(d['angle_params'])
    s.n_torsions = len(d['torsion_atoms']); s.torsion_atoms = i32(d['torsion_atoms']); s.torsion_params = f64(d['torsion_params'])
    s.nb_method = int(d['nb_method']); s.cutoff = float(d['cutoff']); s.switch_distance = float(d['switch_distance'])
    s.rf_dielectric = float(d['rf_dielectric']); s.ewald_alpha = float(d['ewald_alpha'])
    for k in range(3):
        s.pme_grid[k] = int(d['pme_grid'][k])
    s.use_dispersion_correction = int(d['use_dispersion_correction'])
    s.charge = f64(d['charge']); s.sigma = f64(d['sigma']); s.epsilon = f64(d['epsilon'])
    s.n_exceptions = len(d['exception_atoms']); s.exception_atoms = i32(d['exception_atoms'])
    s.exception_params = f64(d['exception_params'])
    s.n_settle = len(d['settle_atoms']); s.settle_atoms = i32(d['settle_atoms'])
    s.settle_dOH, s.settle_dHH = float(d['settle_dOH']), float(d['settle_dHH'])
    s.n_shake = len(d['shake_atoms']); s.shake_atoms = i32(d['shake_atoms']); s.shake_dist = f64(d['shake_dist'])
    s.cmm_frequency = int(d['cmm_frequency'])
    s.n_alch = len(d['alch_atoms']); s.alch_atoms = i32(d['alch_atoms'])
    s.softcore_alpha, s.softcore_a, s.softcore_b, s.softcore_c = [float(v) for v in d['softcore']]
    return s, keep


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _restraint_frames_entry(name, lib_path=None):
    lib = load_library(lib_path)
    if not hasattr(lib, name):
        raise NotImplementedError('%s: this build of the engine library has no pass over stored frames (include/remd_hip_restraints.h is '
                                  'GPU-only)' % name)
    return lib, getattr(lib, name)


def restraint_frames(desc, pos, box, masses, device=0, max_frames_per_launch=0, lib_path=None):
    """(energy [F] kJ/mol at lambda = 1, distance [F] nm) of one restraint at F stored frames (include/remd_hip_restraints.h,
    csrc/restraint_frames.hip).  ``desc``: a dict of forces.restraint_terms (kind, K, r0, atoms1, weights1, atoms2, weights2, periodic;
    weights None: ``masses``), its atom indices addressing the atoms of ``pos`` [F][n_atoms][3] f32; ``box`` [F][3] f32 or None."""
    lib, fn = _restraint_frames_entry('remd_restraint_frames', lib_path)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    if pos.ndim != 3 or pos.shape[2] != 3:
        raise ValueError('pos must be [F][n_atoms][3]')
    F, n_atoms = int(pos.shape[0]), int(pos.shape[1])
    if box is not None:
        box = np.ascontiguousarray(box, dtype=np.float32)
        if box.shape != (F, 3):
            raise ValueError('box must be [F][3] (the edges of a rectangular box; triclinic boxes are not supported)')
    if masses is not None:
        masses = np.ascontiguousarray(masses, dtype=np.float64)
        if masses.shape != (n_atoms,):
            raise ValueError('masses must have one entry per atom of pos')
    a1, a2 = (np.ascontiguousarray(desc['atoms%d' % g], dtype=np.int32).reshape(-1) for g in (1, 2))
    w1, w2 = (None if desc.get('weights%d' % g) is None else np.ascontiguousarray(desc['weights%d' % g], dtype=np.float64).reshape(-1)
              for g in (1, 2))
    for a, w in ((a1, w1), (a2, w2)):
        if w is not None and w.shape != a.shape:
            raise ValueError('a group needs one weight per atom')
    d = RemdRestraintDesc(int(desc['kind']), float(desc['K']), float(desc.get('r0', 0.0)), len(a1), _ip(a1), _dp(w1), len(a2), _ip(a2), _dp(w2),
                          int(desc.get('periodic', 0)), int(desc.get('force_group', 0)))
    energy, distance = np.empty(max(F, 0)), np.empty(max(F, 0))
    rc = fn(int(device), C.byref(d), F, n_atoms, _fp(pos), _fp(box), _dp(masses), int(max_frames_per_launch), _dp(energy), _dp(distance))
    if rc != 0:
        raise RuntimeError('remd_restraint_frames failed (%d): %s' % (rc, lib.remd_last_error(None).decode()))
    return energy, distance


def restraint_frames_last_ms(lib_path=None):
    """Device milliseconds of the kernels of the last restraint_frames call."""
    lib, fn = _restraint_frames_entry('remd_restraint_frames_last_ms', lib_path)
    ms = C.c_double()
    if fn(C.byref(ms)) != 0:
        raise RuntimeError('remd_restraint_frames_last_ms failed: %s' % lib.remd_last_error(None).decode())
    return ms.value


def frame_cvs(cvs, pos, box=None, masses=None, device=0, frames_per_pass=0, lib_path=None, timing=None):
    """values [F][n_cv] f64 (nm, rad) of the collective variables ``cvs`` (multistate.analysis: DistanceCV, AngleCV, DihedralCV, RMSDCV,
    their atom indices addressing the atoms of ``pos``) at F stored frames (include/remd_hip_frame_cvs.h, csrc/frame_cvs.hip): the
    device counterpart of analysis.frame_cvs_numpy, with its arguments and refusals.  ``pos`` [F][n_atoms][3] f32, ``box`` [F][3] f32 or
    None.  The frames are uploaded ``frames_per_pass`` at a time (0: the library's choice); a frame's value does not depend on that.
    ``timing``: a dict that receives 'kernel_ms', the device milliseconds of the kernels of this call."""
    from .multistate import analysis
    lib = load_library(lib_path)
    if not hasattr(lib, 'remd_frame_cvs'):
        raise NotImplementedError('remd_frame_cvs: this build of the engine library has no collective variables of stored frames '
                                  '(include/remd_hip_frame_cvs.h is GPU-only)')
    cvs, pos, box = analysis._check_frames(cvs, pos, box)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    F, n_atoms = int(pos.shape[0]), int(pos.shape[1])
    box = None if box is None else np.ascontiguousarray(box, dtype=np.float32)
    if int(frames_per_pass) < 0:
        raise ValueError('frames_per_pass must not be negative (0: the library chooses)')
    t = analysis.frame_cv_tables(cvs, n_atoms, masses)
    tables = RemdFrameCvTables(len(cvs), _ip(t['kind']), _ip(t['periodic']), _ip(t['cv_groups']), _ip(t['group_off']), _ip(t['atoms']),
                               _dp(t['weights']), _dp(t['reference']))
    out = np.empty((F, len(cvs)))
    ms = C.c_double(0.0)
    rc = lib.remd_frame_cvs(int(device), F, n_atoms, _fp(pos), _fp(box), C.byref(tables), int(frames_per_pass), _dp(out), C.byref(ms))
    if rc != 0:
        raise RuntimeError('remd_frame_cvs failed (%d): %s' % (rc, lib.remd_last_error(None).decode()))
    if timing is not None:
        timing['kernel_ms'] = ms.value
    return out


def _require_exports(lib, names, what):
    for name in names:
        if not hasattr(lib, name):
            raise NotImplementedError('%s: this build of the engine library has no %s' % (name, what))


class _DeviceObject:
    """What the device objects without a HipEngine share: the library and the probe for their entry points, the handle ``h`` made by
    remd_<PREFIX>_create and freed by remd_<PREFIX>_destroy, the check of a return code and the device time of the last call."""
    PREFIX = EXPORTS_NEEDED = MISSING = None

    def __init__(self, lib_path):
        self.lib = load_library(lib_path)
        self.h = None
        _require_exports(self.lib, self.EXPORTS_NEEDED, self.MISSING)

    def _create(self, *args):
        h = C.c_void_p()
        self._check(getattr(self.lib, 'remd_%s_create' % self.PREFIX)(*args, C.byref(h)), 'remd_%s_create' % self.PREFIX)
        self.h = h

    def close(self):
        if self.h is not None:
            getattr(self.lib, 'remd_%s_destroy' % self.PREFIX)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, name):
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (name, rc, self.lib.remd_last_error(None).decode()))

    def last_ms(self):
        """Device milliseconds of the kernels of the last pass."""
        ms = C.c_double()
        self._check(getattr(self.lib, 'remd_%s_last_ms' % self.PREFIX)(self.h, C.byref(ms)), 'remd_%s_last_ms' % self.PREFIX)
        return ms.value


class DeviceMBAR(_DeviceObject):
    """One MBAR problem on the device (include/remd_hip_mbar.h): u_kn [K][N] and N_k are uploaded once; every method is one pass at
    the f_k it is given.  The K x K algebra of the estimator stays with the caller (multistate/analysis.py::MBAR, solver='device')."""

    PREFIX, EXPORTS_NEEDED, MISSING = 'mbar', MBAR_EXPORTS, 'MBAR passes (include/remd_hip_mbar.h is GPU-only)'

    def __init__(self, u_kn, N_k, device=0, lib_path=None):
        super().__init__(lib_path)
        u = np.ascontiguousarray(u_kn, dtype=np.float64)
        nk = np.ascontiguousarray(N_k, dtype=np.int64)
        if u.ndim != 2 or nk.shape != (u.shape[0],):
            raise ValueError('u_kn must be [K][N] and N_k [K]')
        self.K, self.N = int(u.shape[0]), int(u.shape[1])
        self._create(int(device), self.K, self.N, _dp(u), _lp(nk))

    def _f(self, f_k):
        f = np.ascontiguousarray(f_k, dtype=np.float64)
        if f.shape != (self.K,):
            raise ValueError('f_k must have one entry per state')
        return f

    def log_denominator(self, f_k, want_log_den=True):
        """(log_den [N] or None, phi): ln sum_k N_k exp(f_k - u_kn) per sample and the objective sum_n log_den - sum_k N_k f_k."""
        f = self._f(f_k)
        log_den = np.empty(self.N) if want_log_den else None
        phi = C.c_double()
        self._check(self.lib.remd_mbar_log_denominator(self.h, _dp(f), _dp(log_den), C.byref(phi)), 'remd_mbar_log_denominator')
        return log_den, phi.value

    def self_consistent(self, f_k):
        """One application of eq. 11 to every state with the denominator at f_k: f_new [K], not shifted."""
        f = self._f(f_k)
        out = np.empty(self.K)
        self._check(self.lib.remd_mbar_self_consistent(self.h, _dp(f), _dp(out)), 'remd_mbar_self_consistent')
        return out

    def newton_parts(self, f_k):
        """(W_sum [K], W W^T [K][K], phi) at f_k; rows and columns of unsampled states are 0."""
        f = self._f(f_k)
        w, g, phi = np.empty(self.K), np.empty((self.K, self.K)), C.c_double()
        self._check(self.lib.remd_mbar_newton_parts(self.h, _dp(f), _dp(w), _dp(g), C.byref(phi)), 'remd_mbar_newton_parts')
        return w, g, phi.value

    def gram(self, f_k, with_observable=False):
        """W^T W over all K states, [K][K]; with_observable: ([2K][2K] with the u-weighted columns, log_cA [K])."""
        f = self._f(f_k)
        c = 2 * self.K if with_observable else self.K
        g = np.empty((c, c))
        log_cA = np.empty(self.K) if with_observable else None
        self._check(self.lib.remd_mbar_gram(self.h, _dp(f), int(bool(with_observable)), _dp(g), _dp(log_cA)), 'remd_mbar_gram')
        return (g, log_cA) if with_observable else g

    def augmented_gram(self, f_k, u_ln=None, A_in=None, obs_state=None):
        """(f_l [L], log_cA [I], gram [C][C]) over the K stored states, the L perturbed states ``u_ln`` [L][N] and the I observables
        ``A_in`` [I][N] (positive), observable i on the weights of column ``obs_state[i]`` < K + L; C = K + L + I.  Either of ``u_ln``
        and ``A_in`` may be None.  NotImplementedError where the library lacks remd_mbar_augmented_gram."""
        _require_exports(self.lib, MBAR_AUGMENTED_EXPORTS, 'augmented Gram pass (include/remd_hip_mbar.h declares it)')
        f = self._f(f_k)
        u = None if u_ln is None else np.ascontiguousarray(u_ln, dtype=np.float64)
        A = None if A_in is None else np.ascontiguousarray(A_in, dtype=np.float64)
        for a, what in ((u, 'u_ln'), (A, 'A_in')):
            if a is not None and (a.ndim != 2 or a.shape[1] != self.N):
                raise ValueError('%s must be [.][N] with N = %d' % (what, self.N))
        L = 0 if u is None else int(u.shape[0])
        I = 0 if A is None else int(A.shape[0])
        obs = None
        if I:
            obs = np.ascontiguousarray(obs_state, dtype=np.int32).reshape(-1)
            if obs.shape != (I,):
                raise ValueError('obs_state must name one column per observable')
        c = self.K + L + I
        f_l, log_cA, g = np.empty(L), np.empty(I), np.empty((c, c))
        self._check(self.lib.remd_mbar_augmented_gram(self.h, _dp(f), L, _dp(u) if L else None, I, _dp(A) if I else None, _ip(obs),
                                                      _dp(f_l) if L else None, _dp(log_cA) if I else None, _dp(g)), 'remd_mbar_augmented_gram')
        return f_l, log_cA, g

    # ---- bootstrap replicates (remd_mbar_bootstrap_*): NotImplementedError where the library lacks them -----------------------------
    def _require_bootstrap(self):
        _require_exports(self.lib, MBAR_BOOTSTRAP_EXPORTS, 'bootstrap passes (include/remd_hip_mbar.h declares them)')

    def _batch(self, reps, f_b):
        reps = np.ascontiguousarray(reps, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(f_b, dtype=np.float64)
        if f.shape != (reps.size, self.K):
            raise ValueError('f_b must be [nb][K], one row per replicate')
        return reps, f

    def bootstrap_max_batch(self):
        """The most replicates one draw may make resident for this problem."""
        self._require_bootstrap()
        nb = C.c_int()
        self._check(self.lib.remd_mbar_bootstrap_max_batch(self.h, C.byref(nb)), 'remd_mbar_bootstrap_max_batch')
        return nb.value

    def bootstrap_draw(self, seed, b0, nb, sample_states=None):
        """Draws the multiplicities of replicates b0 .. b0 + nb - 1 on the device; they stay resident until the next draw."""
        self._require_bootstrap()
        labels = None if sample_states is None else np.ascontiguousarray(sample_states, dtype=np.int32).reshape(-1)
        if labels is not None and labels.shape != (self.N,):
            raise ValueError('sample_states must have one entry per sample')
        self._check(self.lib.remd_mbar_bootstrap_draw(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, _ip(labels), int(b0), int(nb)),
                    'remd_mbar_bootstrap_draw')

    def bootstrap_counts(self, b0, nb):
        """The multiplicities [nb][N] (uint32) of drawn replicates b0 .. b0 + nb - 1."""
        self._require_bootstrap()
        out = np.empty((max(int(nb), 0), self.N), dtype=np.uint32)
        self._check(self.lib.remd_mbar_bootstrap_counts(self.h, int(b0), int(nb), out.ctypes.data_as(C.POINTER(C.c_uint32))),
                    'remd_mbar_bootstrap_counts')
        return out

    def bootstrap_log_denominator(self, reps, f_b, want_log_den=True):
        """(log_den [nb][N] or None, phi [nb]) of the replicates ``reps``, each at its row of ``f_b`` [nb][K]."""
        self._require_bootstrap()
        reps, f = self._batch(reps, f_b)
        log_den = np.empty((reps.size, self.N)) if want_log_den else None
        phi = np.empty(reps.size)
        self._check(self.lib.remd_mbar_bootstrap_log_denominator(self.h, reps.size, _ip(reps), _dp(f), _dp(log_den), _dp(phi)),
                    'remd_mbar_bootstrap_log_denominator')
        return log_den, phi

    def bootstrap_self_consistent(self, reps, f_b):
        """One weighted application of eq. 11 per replicate: f_new [nb][K], not shifted."""
        self._require_bootstrap()
        reps, f = self._batch(reps, f_b)
        out = np.empty((reps.size, self.K))
        self._check(self.lib.remd_mbar_bootstrap_self_consistent(self.h, reps.size, _ip(reps), _dp(f), _dp(out)), 'remd_mbar_bootstrap_self_consistent')
        return out

    def bootstrap_newton_parts(self, reps, f_b):
        """(W_sum [nb][K], W diag(c) W^T [nb][K][K], phi [nb]) per replicate; rows and columns of unsampled states are 0."""
        self._require_bootstrap()
        reps, f = self._batch(reps, f_b)
        w, g, phi = np.empty((reps.size, self.K)), np.empty((reps.size, self.K, self.K)), np.empty(reps.size)
        self._check(self.lib.remd_mbar_bootstrap_newton_parts(self.h, reps.size, _ip(reps), _dp(f), _dp(w), _dp(g), _dp(phi)),
                    'remd_mbar_bootstrap_newton_parts')
        return w, g, phi

    def bootstrap_rows(self, reps, f_b, u_ln=None, A_in=None, obs_state=None):
        """(f_l [nb][L], log_cA [nb][I]) per replicate: the weighted eq. 11 on the perturbed states ``u_ln`` [L][N] and ln sum_n c_n W A
        of the observables ``A_in`` [I][N] (positive) on the weights of column ``obs_state[i]`` < K + L."""
        self._require_bootstrap()
        reps, f = self._batch(reps, f_b)
        u = None if u_ln is None else np.ascontiguousarray(u_ln, dtype=np.float64)
        A = None if A_in is None else np.ascontiguousarray(A_in, dtype=np.float64)
        for a, what in ((u, 'u_ln'), (A, 'A_in')):
            if a is not None and (a.ndim != 2 or a.shape[1] != self.N):
                raise ValueError('%s must be [.][N] with N = %d' % (what, self.N))
        L = 0 if u is None else int(u.shape[0])
        I = 0 if A is None else int(A.shape[0])
        obs = None
        if I:
            obs = np.ascontiguousarray(obs_state, dtype=np.int32).reshape(-1)
            if obs.shape != (I,):
                raise ValueError('obs_state must name one column per observable')
        f_l, log_cA = np.empty((reps.size, L)), np.empty((reps.size, I))
        self._check(self.lib.remd_mbar_bootstrap_rows(self.h, reps.size, _ip(reps), _dp(f), L, _dp(u) if L else None, I, _dp(A) if I else None,
                                                      _ip(obs), _dp(f_l) if L else None, _dp(log_cA) if I else None), 'remd_mbar_bootstrap_rows')
        return f_l, log_cA

    # ---- free energy surfaces over binned samples (remd_mbar_pmf*): NotImplementedError where the library lacks them ------------------
    def _require_pmf(self):
        _require_exports(self.lib, MBAR_PMF_EXPORTS, 'passes over binned samples (include/remd_hip_mbar.h declares them)')

    def _binned(self, u_n, bin_n):
        u = np.ascontiguousarray(u_n, dtype=np.float64)
        bins = np.ascontiguousarray(bin_n, dtype=np.int32)
        if u.shape != (self.N,) or bins.shape != (self.N,):
            raise ValueError('u_n and bin_n must be [N] with N = %d' % self.N)
        return u, bins

    def pmf_chunk(self):
        """The samples of one bin that one workgroup of the passes over binned samples reduces."""
        self._require_pmf()
        c = C.c_int64()
        self._check(self.lib.remd_mbar_pmf_chunk(self.h, C.byref(c)), 'remd_mbar_pmf_chunk')
        return c.value

    def pmf(self, f_k, u_n, bin_n, nbins, want_all=False):
        """(f_i [nbins], cross [K][nbins], diag [nbins], all_parts [2 + K + nbins] or None) at f_k: the free energies of the bins
        ``bin_n`` [N] (-1: in no bin) of the state ``u_n`` [N] (+inf for an empty bin), sum_{n in i} W_nk W_n,i, sum_{n in i} W_n,i^2 and
        the parts of the column over all binned samples (its f, its self-product, its K and its nbins cross terms)."""
        self._require_pmf()
        f = self._f(f_k)
        u, bins = self._binned(u_n, bin_n)
        nb = max(int(nbins), 0)
        f_i, cross, diag = np.empty(nb), np.empty((self.K, nb)), np.empty(nb)
        parts = np.empty(2 + self.K + nb) if want_all else None
        self._check(self.lib.remd_mbar_pmf(self.h, _dp(f), _dp(u), _ip(bins), int(nbins), _dp(f_i), _dp(cross), _dp(diag), _dp(parts)), 'remd_mbar_pmf')
        return f_i, cross, diag, parts

    def bootstrap_pmf(self, reps, f_b, u_n, bin_n, nbins):
        """f_i [nb][nbins] of the drawn replicates ``reps``, each with its multiplicities at its row of ``f_b`` [nb][K]."""
        self._require_bootstrap()
        self._require_pmf()
        reps, f = self._batch(reps, f_b)
        u, bins = self._binned(u_n, bin_n)
        out = np.empty((reps.size, max(int(nbins), 0)))
        self._check(self.lib.remd_mbar_bootstrap_pmf(self.h, reps.size, _ip(reps), _dp(f), _dp(u), _ip(bins), int(nbins), _dp(out)),
                    'remd_mbar_bootstrap_pmf')
        return out

    def log_weights(self, f_k):
        """log_W_nk [N][K] at f_k."""
        f = self._f(f_k)
        out = np.empty((self.N, self.K))
        self._check(self.lib.remd_mbar_log_weights(self.h, _dp(f), _dp(out)), 'remd_mbar_log_weights')
        return out

    def chunks(self, C_columns):
        """(column, row, Gram) samples per workgroup; the Gram chunk for a matrix of C_columns columns."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.remd_mbar_chunks(self.h, int(C_columns), C.byref(a), C.byref(b), C.byref(c)), 'remd_mbar_chunks')
        return a.value, b.value, c.value


class DeviceTimeseries(_DeviceObject):
    """One timeseries on the device (include/remd_hip_timeseries.h): A [N] is uploaded once; ``inefficiency`` is one call for any
    number of time origins.  What the host keeps: the choice of the origins, n_effective and its maximum (multistate/analysis.py)."""

    PREFIX, EXPORTS_NEEDED, MISSING = 'timeseries', TIMESERIES_EXPORTS, 'timeseries passes (include/remd_hip_timeseries.h is GPU-only)'

    def __init__(self, A_n, device=0, lib_path=None):
        super().__init__(lib_path)
        A = np.ascontiguousarray(A_n, dtype=np.float64)
        if A.ndim != 1:
            raise ValueError('A_n must be one timeseries [N]')
        self.N = int(A.size)
        self._create(int(device), self.N, _dp(A))

    def inefficiency(self, origins, fast=False, mintime=3):
        """(g [S], status [S], last_lag [S]) of the suffixes A[t:] for t in ``origins``: the statistical inefficiency as
        analysis.statistical_inefficiency defines it; status 1 (and g NaN) where the suffix has no variance; the last lag summed."""
        t = np.ascontiguousarray(origins, dtype=np.int64).reshape(-1)
        S = int(t.size)
        g, status, last = np.empty(S), np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int64)
        self._check(self.lib.remd_timeseries_inefficiency(self.h, S, _lp(t), int(bool(fast)), int(mintime), _dp(g), _ip(status), _lp(last)),
                    'remd_timeseries_inefficiency')
        return g, status, last

    def chunk(self):
        """Samples per workgroup: chunk c of every pass covers the samples [c * chunk, (c + 1) * chunk)."""
        c = C.c_int64()
        self._check(self.lib.remd_timeseries_chunks(self.h, C.byref(c)), 'remd_timeseries_chunks')
        return c.value


ENERGY_STORE_MISSING = 'energy-store passes (include/remd_hip_energy_store.h is GPU-only)'


class DeviceEnergyStore(_DeviceObject):
    """The stored energies of a multistate run on the device (include/remd_hip_energy_store.h), in the reporter's own layouts:
    energies [T][R][S], unsampled [T][R][U] (U 0 or 2; None for 0) and states [T][R] are uploaded once; the effective energies, the
    u_ln / N_l of a selection and the transition counts are one call each."""

    PREFIX, EXPORTS_NEEDED, MISSING = 'energy_store', ENERGY_STORE_EXPORTS, ENERGY_STORE_MISSING

    def __init__(self, energies, unsampled, states, device=0, lib_path=None):
        super().__init__(lib_path)
        e = np.ascontiguousarray(energies, dtype=np.float64)
        st = np.ascontiguousarray(states, dtype=np.int32)
        if e.ndim != 3 or st.shape != e.shape[:2]:
            raise ValueError('energies must be [T][R][S] and states [T][R]')
        if not np.array_equal(st, np.asarray(states)):
            raise ValueError('states must be integers that fit 32 bits')
        self.T, self.R, self.S = (int(n) for n in e.shape)
        u = None
        if unsampled is not None and np.shape(unsampled)[-1] != 0:
            u = np.ascontiguousarray(unsampled, dtype=np.float64)
            if u.ndim != 3 or u.shape[:2] != e.shape[:2]:
                raise ValueError('unsampled must be [T][R][U]')
        self.U = 0 if u is None else int(u.shape[2])
        self._create(int(device), self.T, self.R, self.S, self.U, _dp(e), _dp(u), _ip(st))

    def effective_energy(self, log_weights=None, f_l=None):
        """u_n [T]: the sum over the replicas of the energy in the state each occupies; with log_weights [T][S] and f_l [S] the
        expanded-ensemble correction of SAMS on top (both or neither)."""
        lw = None if log_weights is None else np.ascontiguousarray(log_weights, dtype=np.float64)
        f = None if f_l is None else np.ascontiguousarray(f_l, dtype=np.float64)
        if lw is not None and lw.shape != (self.T, self.S):
            raise ValueError('log_weights must be [T][S]')
        if f is not None and f.shape != (self.S,):
            raise ValueError('f_l must be [S]')
        u_n = np.empty(self.T)
        self._check(self.lib.remd_energy_store_effective_energy(self.h, _dp(lw), _dp(f), _dp(u_n)), 'remd_energy_store_effective_energy')
        return u_n

    def gather_u_ln(self, iterations):
        """(u_ln [U + S][R * n_sel], N_l [U + S]) of the selected iterations: column r * n_sel + j is (iterations[j], replica r)."""
        it = np.ascontiguousarray(iterations, dtype=np.int64).reshape(-1)
        n_sel = int(it.size)
        u_ln = np.zeros([self.U + self.S, self.R * n_sel])
        N_l = np.zeros([self.U + self.S], dtype=np.int64)
        self._check(self.lib.remd_energy_store_gather_u_ln(self.h, n_sel, _lp(it), _dp(u_ln), _lp(N_l)), 'remd_energy_store_gather_u_ln')
        return u_ln, N_l

    def transition_counts(self, t_begin, t_end):
        """n_ij [S][S]: the (iteration, replica) pairs with t_begin <= t < t_end - 1 that go from state i to state j."""
        n_ij = np.zeros([self.S, self.S], dtype=np.int64)
        self._check(self.lib.remd_energy_store_transition_counts(self.h, int(t_begin), int(t_end), _lp(n_ij)),
                    'remd_energy_store_transition_counts')
        return n_ij

    def chunks(self):
        """(iterations per workgroup of the effective-energy pass, tile edge of the gather, pairs per workgroup of the counting passes,
        the most states the counting passes keep an LDS histogram for)."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.remd_energy_store_chunks(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), 'remd_energy_store_chunks')
        return a.value, b.value, c.value, d.value


def series_inefficiency_multiple(A_kn, fast=False, mintime=3, device=0, lib_path=None, first_batch=None):
    """(g, status, last_lag, device ms, samples per workgroup) of K series of one length, A_kn [K][N], in one call of the device
    (remd_series_inefficiency_multiple of include/remd_hip_energy_store.h); ``first_batch``: the lags of the first batch, for tests."""
    lib = load_library(lib_path)
    _require_exports(lib, ENERGY_STORE_EXPORTS, ENERGY_STORE_MISSING)
    A = np.ascontiguousarray(A_kn, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError('A_kn must be [K][N]')
    K, N = (int(n) for n in A.shape)
    g, status, last, ms, chunk = C.c_double(), C.c_int32(), C.c_int64(), C.c_double(), C.c_int64()
    if first_batch is None:
        rc = lib.remd_series_inefficiency_multiple(int(device), K, N, _dp(A), int(bool(fast)), int(mintime), C.byref(g), C.byref(status),
                                                   C.byref(last))
    else:
        rc = lib.remd_series_inefficiency_multiple_batched(int(device), K, N, _dp(A), int(bool(fast)), int(mintime), int(first_batch),
                                                           C.byref(g), C.byref(status), C.byref(last), C.byref(ms), C.byref(chunk))
    if rc != 0:
        raise RuntimeError('remd_series_inefficiency_multiple failed (%d): %s' % (rc, lib.remd_last_error(None).decode()))
    return g.value, status.value, last.value, ms.value, chunk.value


class HipEngine:
    """One libremd_hip.so handle = the batched device-state pool of one GPU (replaces cache.ContextCache,
    openmmtools/cache.py:378-461, for the replica-exchange hot path)."""

    is_device = True

    def __init__(self, device=0, stream=None, lib_path=None, ewald_split=None):
        """ewald_split: how the host classes split the Ewald sum of a PME System for this engine (system.system_to_desc):
        'reference' = OpenMM's rule on the NonbondedForce cutoff, 'auto' = a longer Coulomb range that buys a plane-friendly
        mesh (system.rebalanced_coulomb_cutoff), or a Coulomb range in nm.  Potentials agree to the Ewald tolerance either way.
        None: DEFAULT_EWALD_SPLIT on the device library; 'reference' for another build of the ABI (lib_path: the CPU baseline keeps
        the reference's own split)."""
        if ewald_split is None:
            ewald_split = DEFAULT_EWALD_SPLIT if lib_path is None else 'reference'
        self.ewald_split = ewald_split
        self.lib = load_library(lib_path)
        self.h = C.c_void_p()
        rc = self.lib.remd_create(C.byref(self.h), int(device), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise RuntimeError('remd_create failed (%d): %s' % (rc, self.lib.remd_last_error(None).decode()))
        self.device = device
        self._ctor = (device, stream, lib_path, ewald_split)
        self.N = self.K = self.R = self.R_global = self.r_begin = 0
        self._keep = None

    def spawn(self):
        """Another handle of the same library on the same device and stream (one per group of compatible states:
        multistate/_engine_pool.py)."""
        return type(self)(*self._ctor)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.remd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (what, rc, self.lib.remd_last_error(self.h).decode()))

    # ---- set-up ---------------------------------------------------------------------
    def set_system(self, desc_dict):
        sites = desc_dict.get('virtual_sites')
        if sites is not None and not hasattr(self.lib, 'remd_set_virtual_sites'):       # (before the handle changes)
            raise NotImplementedError('remd_set_virtual_sites: this build of the engine library has no virtual sites '
                                      '(include/remd_hip_vsites.h is GPU-only)')
        s, keep = build_desc(desc_dict)
        # Ewald split (system.system_to_desc(ewald_split=...)): range of the direct-space Coulomb sum, 0 = the cutoff
        self._check(self.lib.remd_set_coulomb_cutoff(self.h, float(desc_dict.get('coulomb_cutoff', 0.0))), 'remd_set_coulomb_cutoff')
        # reaction field as the alchemical factory re-writes it (alchemical_rf_treatment='switched'): c_rf = 0 + switch
        rfw = desc_dict.get('rf_unshifted_switch_width')
        self._check(self.lib.remd_set_reaction_field(self.h, int(rfw is not None), float(rfw or 0.0)), 'remd_set_reaction_field')
        self._check(self.lib.remd_set_alchemical_options(self.h, int(bool(desc_dict.get('annihilate_sterics', False)))), 'remd_set_alchemical_options')
        self._check(self.lib.remd_set_system(self.h, C.byref(s)), 'remd_set_system')
        self.N = int(desc_dict['n_atoms'])
        self.n_virtual_sites = 0
        if sites is not None:                            # virtual sites (system.setVirtualSite; csrc/virtual_sites.hip)
            self.set_virtual_sites(sites)
        self.n_regions = 0
        regions = desc_dict.get('alch_regions')
        if regions is not None:                          # general alchemical regions: the factory's custom forces (alchemy.py:1539-2038)
            keep = []

            def f64(a):
                keep.append(np.ascontiguousarray(a, dtype=np.float64)); return _dp(keep[-1])

            def i32(a):
                keep.append(np.ascontiguousarray(a, dtype=np.int32)); return _ip(keep[-1])
            r = RemdAlchRegionsDesc()
            r.n_atoms = self.N; r.n_regions = len(regions['softcore'])
            r.region_of_atom = i32(regions['region_of_atom']); r.softcore = f64(regions['softcore']); r.annihilate = i32(regions['annihilate'])
            r.n_interactions = len(regions['interactions']); r.interactions = i32(np.asarray(regions['interactions'], dtype=np.int32).reshape(-1, 2))
            r.charge, r.sigma, r.epsilon = f64(regions['charge']), f64(regions['sigma']), f64(regions['epsilon'])
            r.n_exceptions = len(regions['exception_atoms']); r.exception_atoms = i32(np.asarray(regions['exception_atoms'], dtype=np.int32).reshape(-1, 2))
            r.exception_params = f64(np.asarray(regions['exception_params'], dtype=np.float64).reshape(-1, 3))
            r.electrostatics = int(regions['electrostatics'])
            r.elec_alpha, r.elec_krf, r.elec_crf = float(regions['elec_alpha']), float(regions['elec_krf']), float(regions['elec_crf'])
            r.elec_switch_distance = float(regions['elec_switch_distance'])
            r.exact_pme = int(regions.get('exact_pme', 0))
            r.consistent_exceptions = int(regions.get('consistent_exceptions', 0))
            for kind, width, npar in (('bond', 2, 2), ('angle', 3, 2), ('torsion', 4, 3)):
                atoms = np.asarray(regions.get(kind + '_atoms', np.zeros((0, width))), dtype=np.int32).reshape(-1, width)
                setattr(r, 'n_%ss' % kind, len(atoms))
                setattr(r, kind + '_atoms', i32(atoms))
                setattr(r, kind + '_params', f64(np.asarray(regions.get(kind + '_params', np.zeros((0, npar))), dtype=np.float64).reshape(-1, npar)))
                setattr(r, kind + '_region', i32(np.asarray(regions.get(kind + '_region', np.zeros(0)), dtype=np.int32)))
            self._check(self.lib.remd_set_alchemical_regions(self.h, C.byref(r)), 'remd_set_alchemical_regions')
            self.n_regions = int(r.n_regions)
        gb = desc_dict.get('gbsa')
        if gb is not None:                               # GBSAOBCForce of an implicit-solvent system (alchemy.py:2144-2225)
            from .custom_gb import is_default_model
            model = None
            if not is_default_model(gb):                 # another OBC-family model or a periodic cutoff (custom_gb.py): remd_set_gb_model
                if not hasattr(self.lib, 'remd_set_gb_model'):
                    raise NotImplementedError('remd_set_gb_model: this build of the engine library has no GB models other than OBC2 without a cutoff '
                                              '(include/remd_hip_gb.h is GPU-only)')
                model = RemdGbModelDesc(*[float(gb[k]) for k in ('offset', 'alpha', 'beta', 'gamma', 'ke', 'surface', 'probe')],
                                        int(gb['method']), float(gb['cutoff']))
            arrs = [np.ascontiguousarray(gb[k], dtype=np.float64) for k in ('charge', 'radius', 'scale')]
            alch = np.ascontiguousarray(gb.get('alchemical', np.zeros(self.N)), dtype=np.int32)
            g = RemdGbsaDesc(self.N, _dp(arrs[0]), _dp(arrs[1]), _dp(arrs[2]), _ip(alch), float(gb['solute_dielectric']), float(gb['solvent_dielectric']),
                             int(gb.get('surface_area', 1)))
            self._check(self.lib.remd_set_gbsa(self.h, C.byref(g)), 'remd_set_gbsa')
            if model is not None:
                self._check(self.lib.remd_set_gb_model(self.h, C.byref(model)), 'remd_set_gb_model')
        if 'force_groups' in desc_dict:                  # Force.getForceGroup() of the force classes (V<g> substeps)
            self.set_force_groups(desc_dict['force_groups'])
        self.n_restraints = 0
        restraints = desc_dict.get('restraints')
        if restraints:                                   # receptor-ligand restraints (forces.py; csrc/restraints.hip)
            self.set_restraints([restraints[k] for k in sorted(restraints)])
        self.n_custom = self.n_custom_globals = self.n_custom_cvs = 0
        self._custom_lrc = None
        self.custom_derivative_names = []
        custom = desc_dict.get('custom_terms')
        if custom:                                       # custom bond / angle / torsion / external forces (custom_expr.py; csrc/custom_terms.hip)
            terms = [custom[k] for k in sorted(custom)]
            self.set_custom_terms(terms)
            if terms[0].get('derivative_columns') is not None and len(terms[0]['derivative_columns']):
                self.set_custom_parameter_derivatives(terms[0]['derivative_columns'], [t.get('derivative_mask', 0) for t in terms],
                                                      terms[0]['derivative_names'])

    def set_virtual_sites(self, sites):
        """The site table of the system (system.system_to_desc's 'virtual_sites': site, kind, parent, weight); after set_system,
        which forgets it."""
        if not hasattr(self.lib, 'remd_set_virtual_sites'):
            raise NotImplementedError('remd_set_virtual_sites: this build of the engine library has no virtual sites '
                                      '(include/remd_hip_vsites.h is GPU-only)')
        site, kind = np.asarray(sites['site']).reshape(-1), np.asarray(sites['kind']).reshape(-1)
        parent = np.asarray(sites['parent']).reshape(len(site), 3)
        weight = np.asarray(sites['weight'], dtype=np.float64).reshape(len(site), 3)
        arr = (RemdVsiteDesc * max(1, len(site)))()
        for k in range(len(site)):
            arr[k].kind, arr[k].site = int(kind[k]), int(site[k])
            for q in range(3):
                arr[k].parent[q] = int(parent[k, q]); arr[k].weight[q] = float(weight[k, q])
        self._check(self.lib.remd_set_virtual_sites(self.h, arr, len(site)), 'remd_set_virtual_sites')
        self.n_virtual_sites = len(site)

    def _restraint_entry(self, name):
        if not hasattr(self.lib, name):
            raise NotImplementedError('%s: this build of the engine library has no restraints (include/remd_hip_restraints.h is GPU-only)' % name)
        return getattr(self.lib, name)

    def set_restraints(self, restraints):
        """The restraints of the system (dicts of system.system_to_desc's 'restraints'); after set_system, which forgets them."""
        fn = self._restraint_entry('remd_set_restraints')
        arr = (RemdRestraintDesc * max(1, len(restraints)))()
        keep = []
        for k, r in enumerate(restraints):
            a1, a2 = (np.ascontiguousarray(r['atoms%d' % g], dtype=np.int32) for g in (1, 2))
            w1, w2 = (np.ascontiguousarray(r['weights%d' % g], dtype=np.float64) for g in (1, 2))
            keep += [a1, a2, w1, w2]
            arr[k] = RemdRestraintDesc(int(r['kind']), float(r['K']), float(r['r0']), len(a1), _ip(a1), _dp(w1), len(a2), _ip(a2), _dp(w2),
                                       int(r['periodic']), int(r['force_group']))
        self._check(fn(self.h, arr, len(restraints)), 'remd_set_restraints')
        self.n_restraints = len(restraints)

    def set_restraint_lambdas(self, lam):
        """[K][n_restraints]: every state's value of each restraint's controlling parameter (after set_states)."""
        fn = self._restraint_entry('remd_set_restraint_lambdas')
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(self.K, self.n_restraints)
        self._check(fn(self.h, _dp(lam)), 'remd_set_restraint_lambdas')

    def restraint_energies(self):
        """[R_local][n_restraints] unscaled restraint energies (kJ/mol) at the current positions."""
        fn = self._restraint_entry('remd_get_restraint_energies')
        out = np.zeros((self.R, self.n_restraints))
        self._check(fn(self.h, _dp(out)), 'remd_get_restraint_energies')
        return out

    def _custom_entry(self, name):
        if not hasattr(self.lib, name):
            raise NotImplementedError('%s: this build of the engine library has no custom bond / angle / torsion / external forces and no compound-bond forces, '
                                      'centroid-bond forces or nonbonded custom forces, nor CMAP torsion forces, donor-acceptor forces, many-particle forces or Generalized-Born expressions '
                                      '(include/remd_hip_custom.h is GPU-only)' % name)
        return getattr(self.lib, name)

    def set_custom_terms(self, terms):
        """The custom forces of the system (dicts of system.system_to_desc's 'custom_terms'); after set_system, which forgets them."""
        fn = self._custom_entry('remd_set_custom_terms')
        n_cv = sum(len(t['cv_offsets']) - 1 for t in terms if 'cv_offsets' in t)
        if n_cv:
            self._custom_cv_entry('remd_get_custom_cv_values')
        arr = (RemdCustomForceDescGB * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            atoms = np.ascontiguousarray(t['atoms'], dtype=np.int32)
            nonbonded = 'excl_offsets' in t                          # a nonbonded force: no atoms, one parameter row per particle
            params = np.ascontiguousarray(t['params'], dtype=np.float64)
            n_terms = len(params) if nonbonded else len(t['donor_atoms']) if 'donor_atoms' in t else len(atoms)
            params = params.reshape(n_terms, -1) if params.size or n_terms else np.zeros((n_terms, 0))
            n_particles = int(t.get('n_particles', 0))               # a compound-bond force: atoms [n][n_particles]
            program = np.ascontiguousarray(t['program'], dtype=np.int32).reshape(-1, 2)
            consts = np.ascontiguousarray(t['consts'], dtype=np.float64)
            defaults = np.ascontiguousarray(t['global_defaults'], dtype=np.float64)
            keep += [atoms, params, program, consts, defaults]
            groups = (0, None, None, None)
            if 'group_offsets' in t:                                 # a centroid-bond force: atoms holds group numbers
                g_off = np.ascontiguousarray(t['group_offsets'], dtype=np.int32)
                g_atoms = np.ascontiguousarray(t['group_atoms'], dtype=np.int32)
                g_w = np.ascontiguousarray(t['group_weights'], dtype=np.float64)
                keep += [g_off, g_atoms, g_w]
                groups = (len(g_off) - 1, _ip(g_off), _ip(g_atoms), _dp(g_w))
            pairs = (0, 0.0, -1.0, None, None, 0)
            if nonbonded:
                e_off = np.ascontiguousarray(t['excl_offsets'], dtype=np.int32)
                e_atoms = np.ascontiguousarray(t['excl_atoms'], dtype=np.int32)
                keep += [e_off, e_atoms]
                pairs = (int(t['nb_method']), float(t['cutoff']), float(t['switch_distance']), _ip(e_off), _ip(e_atoms) if len(e_atoms) else None,
                         int(t['long_range_correction']))
            cvs = (0, None, None, None)
            if 'cv_offsets' in t:                                    # a collective-variable force: one term, no atoms of its own
                c_off = np.ascontiguousarray(t['cv_offsets'], dtype=np.int32)
                c_atoms = np.ascontiguousarray(t['cv_atoms'], dtype=np.int32)
                c_ref = np.ascontiguousarray(t['cv_reference'], dtype=np.float64).reshape(-1, 3)
                if len(c_atoms) != c_off[-1] or len(c_ref) != len(c_atoms):
                    raise ValueError('set_custom_terms: cv_atoms and cv_reference must hold cv_offsets[-1] = %d rows' % c_off[-1])
                keep += [c_off, c_atoms, c_ref]
                cvs = (len(c_off) - 1, _ip(c_off), _ip(c_atoms), _dp(c_ref))
                n_terms = 1
            maps = (None, 0, None)
            if 'map_index' in t:                                     # a CMAP force: atoms [n][8], the maps' blocks in consts
                m_index = np.ascontiguousarray(t['map_index'], dtype=np.int32)
                m_off = np.ascontiguousarray(t['map_offsets'], dtype=np.int32)
                if len(m_index) != n_terms:
                    raise ValueError('set_custom_terms: map_index must hold one map per term (%d, not %d)' % (n_terms, len(m_index)))
                keep += [m_index, m_off]
                maps = (_ip(m_index), len(m_off), _ip(m_off))
            hbond = (0, 0, None, None, 0, None, 0, None, None, None, 0)
            if 'donor_atoms' in t:                                   # a donor-acceptor force: no atoms or parameters of the common kind
                d_atoms = np.ascontiguousarray(t['donor_atoms'], dtype=np.int32).reshape(-1, 3)
                a_atoms = np.ascontiguousarray(t['acceptor_atoms'], dtype=np.int32).reshape(-1, 3)
                d_par = np.ascontiguousarray(t['donor_params'], dtype=np.float64).reshape(len(d_atoms), -1)
                a_par = np.ascontiguousarray(t['acceptor_params'], dtype=np.float64).reshape(len(a_atoms), -1)
                h_off = np.ascontiguousarray(t['hb_excl_offsets'], dtype=np.int32)
                h_acc = np.ascontiguousarray(t['hb_excl_acceptors'], dtype=np.int32)
                if len(h_off) != len(d_atoms) + 1 or len(h_acc) != h_off[-1]:
                    raise ValueError('set_custom_terms: hb_excl_offsets must hold one row per donor and hb_excl_acceptors hb_excl_offsets[-1] = %d entries' % h_off[-1])
                keep += [d_atoms, a_atoms, d_par, a_par, h_off, h_acc]
                hbond = (len(d_atoms), len(a_atoms), _ip(d_atoms), _ip(a_atoms), d_par.shape[1], _dp(d_par) if d_par.size else None,
                         a_par.shape[1], _dp(a_par) if a_par.size else None, _ip(h_off), _ip(h_acc) if len(h_acc) else None, int(t['particle_mask']))
                pairs = (int(t['nb_method']), float(t['cutoff']), -1.0, None, None, 0)
                params = None
            many = (None, 0, (C.c_uint32 * 3)(), 0)
            if 'permutation_mode' in t:                              # a many-particle force: the nonbonded kind's shape, then its own fields
                m_types = np.ascontiguousarray(t['types'], dtype=np.int32)
                if len(m_types) != n_terms:
                    raise ValueError('set_custom_terms: types must hold one type per particle (%d, not %d)' % (n_terms, len(m_types)))
                keep.append(m_types)
                many = (_ip(m_types), int(t['permutation_mode']), (C.c_uint32 * 3)(*[int(v) for v in t['filters']]), int(t['particle_mask']))
            gb = (None, 0, 0)
            if 'stages' in t:                                        # a Generalized-Born force: the nonbonded kind's shape, then its stage table
                g_stages = np.ascontiguousarray(t['stages'], dtype=np.int32).reshape(-1, 28)
                keep.append(g_stages)
                gb = (_ip(g_stages), int(t['n_values']), len(g_stages))
            no_atoms = nonbonded or 'cv_offsets' in t or 'donor_atoms' in t
            arr[k] = RemdCustomForceDescGB(int(t['kind']), n_terms, None if no_atoms else _ip(atoms), 0 if params is None else params.shape[1], _dp(params), len(program), _ip(program),
                                         len(consts), _dp(consts), int(t['stack_depth']), len(defaults), _dp(defaults),
                                         int(t['periodic']), int(t['force_group']), n_particles, *groups, *pairs, *cvs, *maps, *hbond, *many, *gb)
        self._check(fn(self.h, arr, len(terms)), 'remd_set_custom_terms')
        self.n_custom = len(terms)
        self.n_custom_cvs = n_cv
        self.n_custom_globals = len(terms[0]['global_defaults']) if terms else 0
        # the long-range corrections of nonbonded forces: host integrals under every state's globals (custom_expr.LongRangeCorrection),
        # handed over behind every set_custom_globals
        self._custom_lrc = (list(terms), {}) if any(t.get('long_range_correction') for t in terms) else None

    def set_custom_globals(self, values):
        """[K][n_globals]: every state's value of each global parameter of the custom forces (after set_states)."""
        fn = self._custom_entry('remd_set_custom_globals')
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(self.K, self.n_custom_globals)
        self._check(fn(self.h, _dp(values)), 'remd_set_custom_globals')
        if getattr(self, '_custom_lrc', None) is not None:
            from .custom_expr import long_range_coefficients
            terms, cache = self._custom_lrc
            coeff = np.ascontiguousarray(long_range_coefficients(terms, values, cache), dtype=np.float64)
            self._check(self._custom_entry('remd_set_custom_lrc')(self.h, _dp(coeff)), 'remd_set_custom_lrc')

    def custom_energies(self):
        """[R_local][n_custom] energy (kJ/mol) of each custom force at the current positions and the replicas' own states."""
        fn = self._custom_entry('remd_get_custom_energies')
        out = np.zeros((self.R, self.n_custom))
        self._check(fn(self.h, _dp(out)), 'remd_get_custom_energies')
        return out

    def _custom_derivative_entry(self, name):
        if not hasattr(self.lib, name):
            raise NotImplementedError('%s: this build of the engine library has no energy parameter derivatives of custom forces '
                                      '(addEnergyParameterDerivative: the entry points of include/remd_hip_custom.h are GPU-only)' % name)
        return getattr(self.lib, name)

    def set_custom_parameter_derivatives(self, columns, force_masks, names=None):
        """The energy parameter derivatives the custom forces declared (custom_expr.custom_terms_desc): the distinct global columns and,
        per custom force, the mask of those it declared; after set_custom_terms, which forgets them."""
        fn = self._custom_derivative_entry('remd_set_custom_parameter_derivatives')
        columns = np.ascontiguousarray(columns, dtype=np.int32).reshape(-1)
        masks = np.ascontiguousarray(force_masks, dtype=np.uint32).reshape(-1)
        if len(masks) != self.n_custom:
            raise ValueError('set_custom_parameter_derivatives: one mask per custom force (%d, not %d)' % (self.n_custom, len(masks)))
        self._check(fn(self.h, columns.ctypes.data_as(C.POINTER(C.c_int32)), len(columns), masks.ctypes.data_as(C.POINTER(C.c_uint32))),
                    'remd_set_custom_parameter_derivatives')
        self.custom_derivative_names = [str(n) for n in names] if names is not None else ['column %d' % c for c in columns]

    def custom_energy_parameter_derivatives(self):
        """[R_local][n_derivatives]: dE/dparameter (kJ/mol per unit of the parameter) of the global parameters the custom forces declared
        with addEnergyParameterDerivative, summed over the forces that declared each, at the current positions and each replica's own
        state's globals (OpenMM's State.getEnergyParameterDerivatives); the columns are ``custom_derivative_names``."""
        fn = self._custom_derivative_entry('remd_get_custom_parameter_derivatives')
        names = getattr(self, 'custom_derivative_names', [])
        if not names:
            raise ValueError('custom_energy_parameter_derivatives: no custom force of the system declares an energy parameter derivative '
                             '(addEnergyParameterDerivative)')
        out = np.zeros((self.R, len(names)))
        self._check(fn(self.h, _dp(out)), 'remd_get_custom_parameter_derivatives')
        return out

    def custom_energy_parameter_derivatives_at_states(self):
        """[R_local][K][n_derivatives]: the same derivatives (kJ/mol per unit of the parameter) at the current positions under the globals
        of every thermodynamic state, unsampled ones included -- ``[r][label_r]`` is bit-identical to
        ``custom_energy_parameter_derivatives()[r]``; the columns are ``custom_derivative_names``.  One call: whatever depends on the
        positions alone (centroids, candidate pairs, neighbour rows) is computed once for all K states."""
        fn = self._custom_derivative_entry('remd_get_custom_parameter_derivatives_at_states')
        names = getattr(self, 'custom_derivative_names', [])
        if not names:
            raise ValueError('custom_energy_parameter_derivatives_at_states: no custom force of the system declares an energy parameter '
                             'derivative (addEnergyParameterDerivative)')
        out = np.zeros((self.R, self.K, len(names)))
        self._check(fn(self.h, _dp(out)), 'remd_get_custom_parameter_derivatives_at_states')
        return out

    def _custom_cv_entry(self, name):
        if not hasattr(self.lib, name):
            raise NotImplementedError('%s: this build of the engine library has no collective-variable forces (CustomCVForce / RMSDForce: '
                                      'REMD_CUSTOM_CV of include/remd_hip_custom.h is GPU-only)' % name)
        return getattr(self.lib, name)

    def custom_cv_values(self):
        """[R_local][total collective variables]: the current RMSDs (nm) of the CustomCVForce / RMSDForce forces, in the order of
        the forces and of the variables within one (OpenMM's getCollectiveVariableValues)."""
        fn = self._custom_cv_entry('remd_get_custom_cv_values')
        if not getattr(self, 'n_custom_cvs', 0):
            raise ValueError('custom_cv_values: the system has no CustomCVForce or RMSDForce')
        out = np.zeros((self.R, self.n_custom_cvs))
        self._check(fn(self.h, _dp(out)), 'remd_get_custom_cv_values')
        return out

    def set_states(self, beta, lambda_sterics=None, lambda_electrostatics=None, energy_const=None):
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64)
                for a in (lambda_sterics, lambda_electrostatics, energy_const)]
        self._check(self.lib.remd_set_states(self.h, len(beta), _dp(beta), *[_dp(a) for a in arrs]), 'remd_set_states')
        self.K = len(beta)

    def set_region_lambdas(self, lambda_sterics, lambda_electrostatics):
        """[K][n_regions] lambdas of general alchemical regions (after set_states)."""
        ls = np.ascontiguousarray(lambda_sterics, dtype=np.float64).reshape(self.K, -1)
        le = np.ascontiguousarray(lambda_electrostatics, dtype=np.float64).reshape(self.K, -1)
        self._check(self.lib.remd_set_region_lambdas(self.h, self.K, ls.shape[1], _dp(ls), _dp(le)), 'remd_set_region_lambdas')

    def set_region_bonded_lambdas(self, lambda_bonds=None, lambda_angles=None, lambda_torsions=None):
        """[K][n_regions] lambdas of the alchemically softened bonded terms (after set_region_lambdas; None: 1)."""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(self.K, -1) for a in (lambda_bonds, lambda_angles, lambda_torsions)]
        n = next((a.shape[1] for a in arrs if a is not None), self.n_regions)
        self._check(self.lib.remd_set_region_bonded_lambdas(self.h, self.K, n, *[_dp(a) for a in arrs]), 'remd_set_region_bonded_lambdas')

    def set_integrator(self, splitting, timestep, collision_rate, n_steps, reassign_velocities=True,
                       constraint_tolerance=1e-8):
        self._check(self.lib.remd_set_integrator(self.h, splitting.encode(), float(timestep), float(collision_rate),
                                                 int(n_steps), int(bool(reassign_velocities)),
                                                 float(constraint_tolerance)), 'remd_set_integrator')

    def set_work_measurement(self, measure_heat=False, measure_shadow_work=False):
        """LangevinIntegrator(measure_heat=, measure_shadow_work=) (integrators.py:1077-1125)."""
        self._check(self.lib.remd_set_work_measurement(self.h, int(bool(measure_heat)), int(bool(measure_shadow_work))), 'remd_set_work_measurement')

    def get_work(self):
        """dict(heat, shadow_work [kJ/mol], n_accepted, n_trials) per local replica, accumulated since the last reset_work."""
        heat, sw = np.zeros(self.R), np.zeros(self.R)
        na, nt = np.zeros(self.R, np.int64), np.zeros(self.R, np.int64)
        self._check(self.lib.remd_get_work(self.h, _dp(heat), _dp(sw), _lp(na), _lp(nt)), 'remd_get_work')
        return dict(heat=heat, shadow_work=sw, n_accepted=na, n_trials=nt)

    def reset_work(self):
        self._check(self.lib.remd_reset_work(self.h), 'remd_reset_work')

    def set_force_groups(self, groups):
        """Force groups of (external, bonds, angles, torsions, nonbonded direct, PME reciprocal) for V<g> substeps."""
        g = (C.c_int32 * 6)(*[int(x) for x in groups])
        self._check(self.lib.remd_set_force_groups(self.h, g), 'remd_set_force_groups')

    # ---- sharding through RCCL inside the library (include/remd_hip.h; a torch.distributed host may use multistate/comm.py) ----
    def comm_unique_id(self):
        """Rank 0: the 128 opaque bytes every other rank needs for ``comm_init`` (passed on by the host's own channel)."""
        buf = (C.c_ubyte * 128)()
        self._check(self.lib.remd_comm_unique_id(buf), 'remd_comm_unique_id')
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        if len(unique_id) != 128:
            raise ValueError('the communicator id is 128 bytes')
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._check(self.lib.remd_comm_init(self.h, int(rank), int(world), buf), 'remd_comm_init')

    def comm_all_gather_energies(self):
        """After ``compute_energies`` into the handle's own matrix: every other rank's rows, on the handle's stream."""
        self._check(self.lib.remd_comm_all_gather_energies(self.h), 'remd_comm_all_gather_energies')

    def comm_finalize(self):
        self._check(self.lib.remd_comm_finalize(self.h), 'remd_comm_finalize')

    def set_restart_attempts(self, n):
        """mcmc.py:706-759: retries of a move whose result holds a NaN (restored start state, fresh noise)."""
        self._check(self.lib.remd_set_restart_attempts(self.h, int(n)), 'remd_set_restart_attempts')

    def set_barostat(self, pressure, frequency=25):
        """Monte Carlo barostat of the NPT states (states.py:1177-1181): pressure per state in kJ/mol/nm^3, or None."""
        if pressure is None:
            self._check(self.lib.remd_set_barostat(self.h, 0, None, 0), 'remd_set_barostat')
            return
        p = np.ascontiguousarray(pressure, dtype=np.float64)
        self._check(self.lib.remd_set_barostat(self.h, len(p), _dp(p), int(frequency)), 'remd_set_barostat')

    def _barostat_axis_entry(self, name):
        if not hasattr(self.lib, name):
            raise NotImplementedError('%s: this build of the engine library has no per-axis barostats (include/remd_hip_barostat.h is GPU-only)' % name)
        return getattr(self.lib, name)

    def set_barostat_axes(self, pressure, surface_tension, kind, xy_or_scale_mask, zmode=0, frequency=25):
        """MonteCarloAnisotropicBarostat (kind BAROSTAT_ANISOTROPIC, xy_or_scale_mask = scaleX | scaleY << 1 | scaleZ << 2) or
        MonteCarloMembraneBarostat (kind BAROSTAT_MEMBRANE, xy_or_scale_mask = the xy mode, zmode the z mode) of the states: pressure
        per state in kJ/mol/nm^3, surface tension per state in kJ/mol/nm^2 (None: 0).  set_barostat returns to the isotropic move."""
        fn = self._barostat_axis_entry('remd_set_barostat_axes')
        p = np.ascontiguousarray(pressure, dtype=np.float64)
        g = None if surface_tension is None else np.ascontiguousarray(surface_tension, dtype=np.float64)
        if g is not None and g.shape != p.shape:
            raise ValueError('one surface tension per state')
        self._check(fn(self.h, len(p), _dp(p), _dp(g), int(kind), int(xy_or_scale_mask), int(zmode), int(frequency)), 'remd_set_barostat_axes')

    def barostat_axis_stats(self):
        """(volume step [R][3], attempted [R][3], accepted [R][3]) of the per-axis barostat, axes x, y, z."""
        fn = self._barostat_axis_entry('remd_get_barostat_axis_stats')
        vs = np.zeros((self.R, 3)); na = np.zeros((self.R, 3), np.int64); nc = np.zeros((self.R, 3), np.int64)
        self._check(fn(self.h, _dp(vs), na.ctypes.data_as(c_int64_p), nc.ctypes.data_as(c_int64_p)), 'remd_get_barostat_axis_stats')
        return vs, na, nc

    def set_energy_const_volume(self, volume):
        """The energy constants of set_states scale as volume / V with the replica's box (NPT + alchemical states)."""
        self._check(self.lib.remd_set_energy_const_volume(self.h, float(volume)), 'remd_set_energy_const_volume')

    def get_boxes(self):
        box = np.zeros((self.R, 3), dtype=np.float64)
        self._check(self.lib.remd_get_boxes(self.h, _dp(box)), 'remd_get_boxes')
        return box

    def barostat_attempts(self, n_attempts):
        """mcmc.py:1597-1700 MonteCarloBarostatMove: n volume moves of every local replica outside the integrator."""
        self._check(self.lib.remd_barostat_attempts(self.h, int(n_attempts)), 'remd_barostat_attempts')

    def mc_rigid_moves(self, moves, iteration):
        """mcmc.py:1704-1910 MCDisplacementMove / MCRotationMove with proposal='device': the moves in order for every local
        replica, entirely on the device (include/remd_hip_mcmoves.h).  ``moves``: (kind, atom indices, sigma in nm, place in the
        flattened sequence) each; returns the accepted flags, [n_moves][R_local] of 0 / 1."""
        if not hasattr(self.lib, 'remd_mc_rigid_moves'):
            raise NotImplementedError('remd_mc_rigid_moves: this build of the engine library has no Monte Carlo moves on the device '
                                      '(include/remd_hip_mcmoves.h is GPU-only)')
        arr = (RemdMcMoveDesc * max(1, len(moves)))()
        keep = []
        for k, (kind, atoms, sigma, position) in enumerate(moves):
            a = np.ascontiguousarray(atoms, dtype=np.int32).reshape(-1)
            keep.append(a)
            arr[k].kind, arr[k].n_atoms, arr[k].atoms = int(kind), len(a), a.ctypes.data_as(c_int32_p)
            arr[k].sigma_nm, arr[k].position = float(sigma), int(position)
        accepted = np.zeros((max(1, len(moves)), max(1, self.R)), dtype=np.int32)     # (never empty: the library names what it refuses)
        self._check(self.lib.remd_mc_rigid_moves(self.h, arr, len(moves), int(iteration), accepted.ctypes.data_as(c_int32_p)),
                    'remd_mc_rigid_moves')
        return accepted[:len(moves), :self.R]

    def barostat_stats(self):
        vs = np.zeros(self.R); na = np.zeros(self.R, np.int64); nc = np.zeros(self.R, np.int64)
        self._check(self.lib.remd_get_barostat_stats(self.h, _dp(vs), na.ctypes.data_as(c_int64_p), nc.ctypes.data_as(c_int64_p)),
                    'remd_get_barostat_stats')
        return vs, na, nc

    def minimize(self, tolerance=1.0, max_iterations=0):
        """FIRE minimisation of every local replica (multistatesampler.py:611-647).  tolerance in kJ/mol/nm.
        Returns (converged flags, FIRE steps taken)."""
        conv = np.zeros(self.R, dtype=np.int32)
        n = C.c_int32(0)
        self._check(self.lib.remd_minimize(self.h, float(tolerance), int(max_iterations), conv.ctypes.data_as(c_int32_p),
                                           C.byref(n)), 'remd_minimize')
        return conv, n.value

    def set_replicas(self, R_global, r_begin, x, v, box, labels):
        """x = None sizes the handle for len(box) replicas whose coordinates follow through copy_replicas."""
        box = np.ascontiguousarray(box, dtype=np.float64)
        R_local = box.reshape(-1, 3).shape[0] if x is None else np.shape(x)[0]
        x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        box = box.reshape(R_local, 3)
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        assert (x is None or x.shape == (R_local, self.N, 3)) and labels.shape == (R_global,)
        self._check(self.lib.remd_set_replicas(self.h, int(R_global), int(r_begin), R_local, _dp(x), _dp(v),
                                               _dp(box), _lp(labels)), 'remd_set_replicas')
        self.R, self.R_global, self.r_begin = R_local, int(R_global), int(r_begin)

    POSITIONS, VELOCITIES, BOXES = 1, 2, 4

    def copy_replicas(self, slots, source, source_slots, what=7):
        """Positions / velocities / boxes (bits 1 / 2 / 4 of ``what``) of ``source``'s local replicas ``source_slots`` into this
        handle's local replicas ``slots``, device to device (remd_copy_replicas; one handle per compatibility group)."""
        d = np.ascontiguousarray(slots, dtype=np.int32)
        s = np.ascontiguousarray(source_slots, dtype=np.int32)
        if d.shape != s.shape or d.ndim != 1:
            raise ValueError('one source slot per destination slot')
        self._check(self.lib.remd_copy_replicas(self.h, d.ctypes.data_as(c_int32_p), source.h, s.ctypes.data_as(c_int32_p),
                                                int(len(d)), int(what)), 'remd_copy_replicas')

    def set_replica_ids(self, ids):
        """Global replica indices that key the local replicas' random streams (a handle holding a non-contiguous subset of the
        ensemble: multistate/_engine_pool.py); None restores r_begin + r.  Call after set_replicas."""
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        if ids is not None and ids.shape != (self.R,):
            raise ValueError('one id per local replica')
        self._check(self.lib.remd_set_replica_ids(self.h, _lp(ids)), 'remd_set_replica_ids')

    def set_labels(self, labels):
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        self._check(self.lib.remd_set_labels(self.h, _lp(labels)), 'remd_set_labels')

    def seed(self, seed):
        self._check(self.lib.remd_seed(self.h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)), 'remd_seed')

    # ---- hot path ----------------------------------------------------------------------
    def propagate(self, iteration):
        flags = np.zeros(self.R, dtype=np.int32)
        self._check(self.lib.remd_propagate(self.h, int(iteration), _ip(flags)), 'remd_propagate')
        return flags

    def constraint_stats(self):
        """(most Newton updates an X-H position solve has needed, whether one ever reached the bound unconverged)"""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.remd_get_constraint_stats(self.h, C.byref(a), C.byref(b)), 'remd_get_constraint_stats')
        return int(a.value), bool(b.value)

    def set_phases(self, n):
        """remd_set_phases: 0 = by rule (two blocks of replicas whose MD steps take turns when the process keeps few hardware queues),
        1 = one block, 2 = two blocks"""
        self._check(self.lib.remd_set_phases(self.h, int(n)), 'remd_set_phases')

    def phases_active(self):
        """blocks the last propagate ran as"""
        n = C.c_int32(1)
        self._check(self.lib.remd_get_phases(self.h, C.byref(n)), 'remd_get_phases')
        return int(n.value)

    @staticmethod
    def propagate_many(engines, iteration):
        """remd_propagate_many: the engines' MD steps take turns on one device from one host thread; returns the NaN flags per engine"""
        lib = engines[0].lib
        hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
        flags = np.zeros(sum(e.R for e in engines), dtype=np.int32)
        engines[0]._check(lib.remd_propagate_many(hs, len(engines), int(iteration), _ip(flags)), 'remd_propagate_many')
        return np.split(flags, np.cumsum([e.R for e in engines])[:-1])

    def compute_energies(self, d_rows=None, want_host=True, want_potential=False):
        """Rows [R_local, K] of u_kl.  d_rows: device pointer (int) or None for the handle's matrix."""
        ukl = np.empty((self.R, self.K), dtype=np.float64) if want_host else None
        pot = np.empty(self.R, dtype=np.float64) if want_potential else None
        self._check(self.lib.remd_compute_energies(self.h, C.c_void_p(d_rows) if d_rows else None, _dp(ukl), _dp(pot)),
                    'remd_compute_energies')
        return (ukl, pot) if want_potential else ukl

    def ukl_device_ptr(self):
        p = C.c_void_p()
        self._check(self.lib.remd_ukl_device_ptr(self.h, C.byref(p)), 'remd_ukl_device_ptr')
        return p.value

    def mix(self, scheme, iteration, labels, d_ukl=None, R=None, K=None, ld=0, log_weights=None):
        R = self.R_global if R is None else R
        K = self.K if K is None else K
        labels = np.ascontiguousarray(labels, dtype=np.int64).copy()
        nacc = np.zeros((K, K), dtype=np.int64)
        nprop = np.zeros((K, K), dtype=np.int64)
        sid = MIX_SCHEMES[scheme]
        logw = None if log_weights is None else np.ascontiguousarray(log_weights, dtype=np.float64)
        logP = np.zeros((R, K), dtype=np.float64) if sid == 3 else None
        self._check(self.lib.remd_mix(self.h, sid, int(iteration), R, K, C.c_void_p(d_ukl) if d_ukl else None,
                                      int(ld), _lp(labels), _lp(nacc), _lp(nprop), _dp(logw), _dp(logP)), 'remd_mix')
        return labels, nacc, nprop, logP

    def mix_host(self, scheme, iteration, ukl, labels, log_weights=None, n_attempts=-1):
        ukl = np.ascontiguousarray(ukl, dtype=np.float64)
        R, K = ukl.shape
        labels = np.ascontiguousarray(labels, dtype=np.int64).copy()
        nacc = np.zeros((K, K), dtype=np.int64)
        nprop = np.zeros((K, K), dtype=np.int64)
        sid = MIX_SCHEMES[scheme]
        logw = None if log_weights is None else np.ascontiguousarray(log_weights, dtype=np.float64)
        logP = np.zeros((R, K), dtype=np.float64) if sid == 3 else None
        self._check(self.lib.remd_mix_host(self.h, sid, int(iteration), R, K, _dp(ukl), _lp(labels), _lp(nacc),
                                           _lp(nprop), _dp(logw), _dp(logP), int(n_attempts)), 'remd_mix_host')
        return labels, nacc, nprop, logP

    # ---- snapshots / hooks ---------------------------------------------------------------
    def get_replicas(self, positions=True, velocities=True, potential=False, kinetic=False):
        x = np.empty((self.R, self.N, 3)) if positions else None
        v = np.empty((self.R, self.N, 3)) if velocities else None
        u = np.empty(self.R) if potential else None
        k = np.empty(self.R) if kinetic else None
        self._check(self.lib.remd_get_replicas(self.h, _dp(x), _dp(v), _dp(u), _dp(k)), 'remd_get_replicas')
        return x, v, u, k

    def get_forces(self, groups=None):
        """Forces [R, N, 3] in kJ/mol/nm.  groups: None (every force) or a bit mask of force groups 0 ... 31, as OpenMM's
        getState(getForces=True, groups=mask)."""
        f = np.empty((self.R, self.N, 3))
        if groups is None:
            self._check(self.lib.remd_get_forces(self.h, _dp(f)), 'remd_get_forces')
        else:
            self._check(self.lib.remd_get_group_forces(self.h, int(groups) & 0xffffffff, _dp(f)), 'remd_get_group_forces')
        return f

    def step(self, splitting, iteration=0, first_step=0, n_steps=1):
        self._check(self.lib.remd_step(self.h, splitting.encode(), int(iteration), int(first_step), int(n_steps)),
                    'remd_step')

    def energy_components(self):
        names = ['external', 'bonds', 'angles', 'torsions', 'exceptions', 'ewald_exclusions', 'pme_reciprocal',
                 'constants', 'nonbonded_direct']
        out = np.zeros((self.R, 9))
        self._check(self.lib.remd_get_energy_components(self.h, _dp(out)), 'remd_get_energy_components')
        return [dict(zip(names, row)) for row in out]

    def test_fft3d(self, data, inverse=False):
        a = np.ascontiguousarray(data, dtype=np.complex64).copy()
        nx, ny, nz = a.shape
        self._check(self.lib.remd_test_fft3d(self.h, nx, ny, nz, a.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                             int(bool(inverse))), 'remd_test_fft3d')
        return a

    def sync(self):
        self._check(self.lib.remd_sync(self.h), 'remd_sync')

    def last_timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.lib.remd_last_timing(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(propagate_ms=a.value, energies_ms=b.value, mix_ms=c.value)

    def roof_microbench(self):
        """Achievable roofs of this box: STREAM triad GB/s, v_fma_f32 and v_pk_fma_f32 TFLOP/s (include/remd_hip.h)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.remd_roof_microbench(self.h, C.byref(a), C.byref(b), C.byref(c)), 'remd_roof_microbench')
        out = dict(stream_triad_gb_per_s=a.value, fma_f32_tflop_per_s=b.value, pk_fma_f32_tflop_per_s=c.value)
        g = C.c_double()
        if self.lib.remd_roof_clock_ghz(self.h, C.byref(g)) == 0 and g.value > 0:
            # 157.3 TFLOP/s = 256 CUs x 4 SIMDs x 32 lanes x 2 flop at 2.4 GHz: what the same issue rate gives at the measured clock
            out['shader_clock_ghz_under_fma_load'] = g.value
            out['fma_f32_peak_at_that_clock_tflop_per_s'] = 157.3 * g.value / 2.4
        return out

    def roof_pair_step(self, waves_per_simd, chains=1, ghz=2.4):
        """(cycles per cluster-pair step per SIMD at `ghz`, microseconds of the launch): the pair kernel's step replayed from registers."""
        c, us = C.c_double(), C.c_double()
        self._check(self.lib.remd_roof_pair_step(self.h, int(waves_per_simd), int(chains), float(ghz), C.byref(c), C.byref(us)), 'remd_roof_pair_step')
        return c.value, us.value

    def profile_enable(self, on=1, kernel_class=None):
        if kernel_class is not None:
            self.lib.remd_profile_filter(self.h, kernel_class.encode())
        self.lib.remd_profile_enable(self.h, int(on))

    def profile_reset(self):
        self.lib.remd_profile_reset(self.h)

    def profile_get(self, name):
        n, ms = C.c_int64(), C.c_double()
        self.lib.remd_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms))
        return n.value, ms.value
