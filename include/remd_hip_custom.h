/*
 * remd_hip_custom.h — GPU-only extension of the C ABI in remd_hip.h: custom bond, angle, torsion, external, compound-bond,
 * centroid-bond, nonbonded, collective-variable, donor-acceptor (hydrogen-bond), many-particle (three-body) and Generalized-Born forces, and CMAP
 * torsion maps.
 *
 * OpenMM's CustomBondForce, CustomAngleForce, CustomTorsionForce and CustomExternalForce: an energy expression of r (bond), theta
 * (angle, torsion) or x, y, z (external), of per-term parameters and of global parameters, evaluated per term.  The host compiles
 * the expression (openmmtools_amd/custom_expr.py) into a postfix program; the device runs it on a small stack machine that carries
 * every value together with its partial derivatives with respect to the force's variables (forward mode), so the forces need no
 * second program.
 *
 * The program: n_program (opcode, operand) pairs of int32.  Operands index the constant table (REMD_CX_CONST), the force's
 * variables (REMD_CX_VAR: 0 = r / theta / x, 1 = y, 2 = z), the term's parameters (REMD_CX_PARAM), the handle's global-parameter
 * columns (REMD_CX_GLOBAL) or give the exponent itself (REMD_CX_POWI: a small constant integer power, evaluated with
 * multiplications).  Every other opcode takes its arguments from the stack, first argument deepest, and pushes one result.
 * Piecewise functions (abs, min, max, select) differentiate as the branch taken; step, delta, floor and ceil have derivative zero.
 *
 * Compound-bond forces (REMD_CUSTOM_COMPOUND, OpenMM's CustomCompoundBondForce): every term joins n_particles particles (1 ...
 * REMD_CUSTOM_MAX_PARTICLES), the variables are their coordinates x1 y1 z1 ... (REMD_CX_VAR operand 3 * particle + component, particle
 * zero-based), and REMD_CX_DISTANCE / REMD_CX_ANGLE / REMD_CX_DIHEDRAL push the distance, angle (0 ... pi) or dihedral (-pi ... pi, the
 * sign convention of PeriodicTorsionForce) of the particle slots packed into the operand, 4 bits each, first argument lowest; they
 * take nothing from the stack and are legal only in such a program.  pointdistance is REMD_CX_PERIODICDISTANCE; it and the differences
 * between particles are minimum images only where the force is periodic.  The device runs the program once per particle slot, each
 * pass carrying the gradient with respect to that particle (csrc/custom_compound.hip).
 *
 * Centroid-bond forces (REMD_CUSTOM_CENTROID, OpenMM's CustomCentroidBondForce): a compound-bond force whose particles are the weighted
 * centroids of groups of atoms.  The descriptor carries the force's n_groups groups in CSR form (group_offsets, group_atoms) with
 * weights that sum to 1 in every group (group_weights); `atoms` holds group numbers, n_particles of them per bond, and the program is a
 * compound-bond program over the centroids x1 y1 z1 ....  A centroid is x_first + sum_i w_i img(x_i - x_first), the differences minimum
 * images under the replica's own box where the force is periodic (the convention of remd_hip_restraints.h: a group whose molecules were
 * wrapped one by one keeps its centroid), summed in f64 in a fixed order.  Per force evaluation the device computes every centroid,
 * runs the bonds over them as it runs compound bonds, and gives atom i of a group -w_i dE/d(centroid) (csrc/custom_centroid.hip).  A
 * group may be named by any number of bonds, an atom may sit in any number of groups.  The restraint forms of remd_hip_restraints.h keep
 * their own entry points.
 *
 * Nonbonded forces (REMD_CUSTOM_NONBONDED, OpenMM's CustomNonbondedForce): the energy is an expression of the distance r of two
 * particles (REMD_CX_VAR 0), summed over every pair i < j that no exclusion names and, with a cutoff, that lies inside it.  n_terms is
 * the system's particle count N, params is [N][n_params] with n_params <= REMD_CUSTOM_MAX_PARAMS / 2, atoms is NULL, and REMD_CX_PARAM
 * operand k is parameter k of the pair's first particle, n_params + k of its second.  nb_method: 0 every pair, 1 a cutoff without and 2
 * with minimum images under the replica's own box (periodic = 1 exactly then; every box edge must stay >= 2 cutoff, also under a
 * barostat).  switch_distance in (0, cutoff) multiplies the energy by OpenMM's switching function 1 - 10 t^3 + 15 t^4 - 6 t^5,
 * t = (r - switch_distance) / (cutoff - switch_distance); < 0: none.  Exclusions in CSR form, symmetric (j in i's row and i in j's),
 * each row sorted.  long_range_correction = 1 (nb_method 2 only): the force's energy gains coeff[state][force] / V, V the replica's own
 * box volume and coeff the host's integral of the expression beyond the cutoff under the state's globals (remd_set_custom_lrc, to be
 * called after every remd_set_custom_globals: the forces refuse to act on coefficients older than the globals); the u_kl rows gain
 * beta_l (coeff_l - coeff_own) / V.  One wavefront per tile of 64 x 64 particles, every tile visited (csrc/custom_nonbonded.hip): the
 * cost is quadratic in N.
 *
 * Collective-variable forces (REMD_CUSTOM_CV, OpenMM's CustomCVForce over RMSDForce variables): the energy is an expression of n_cvs (1 ...
 * REMD_CUSTOM_MAX_CVS) collective variables (REMD_CX_VAR operand 0, 1, 2), each the RMSD in nm of a set of particles from reference
 * coordinates after the optimal superposition: V = sqrt(min over proper rotations U of sum_i |x_i - c - U ref_i|^2 / n), c the centroid of
 * the n particles.  The variables come in CSR form (cv_offsets, cv_atoms) with cv_reference [.][3] beside cv_atoms, the reference of
 * every variable centred on the centroid of its own rows (within 1e-9 nm); a variable has at least 3 particles, none twice; a particle
 * may sit in several variables.  n_terms = 1, atoms NULL, n_params = 0, periodic = 0: no difference is a minimum image (OpenMM's rule),
 * so the particles of a variable must be ones that no barostat moves apart (the host's business: openmmtools_amd refuses a variable
 * that spans molecules of a periodic System).  Per force evaluation the device superposes every variable (f64 sums in a fixed order,
 * the rotation from Horn's quaternion matrix by Jacobi rotations, the deviation summed directly), runs the expression on the RMSDs and
 * gives particle i of variable k -(dE/dV_k) (x_i - c - U ref_i) / (n V_k); a mean square deviation below 1e-20 nm^2 gives V = 0 and no
 * force from that variable (csrc/custom_cv.hip).  remd_get_custom_cv_values reads the RMSDs back.
 *
 * CMAP torsion forces (REMD_CUSTOM_CMAP, OpenMM's CMAPTorsionForce): a term is two dihedrals, phi of the particles atoms[k][0 ... 3] and
 * psi of atoms[k][4 ... 7] (n_particles = 8; the two quadruples usually share particles), each in (-pi, pi] with the sign convention
 * of REMD_CUSTOM_TORSION and of REMD_CX_DIHEDRAL, and its energy is map map_index[k] of the force at (phi, psi).  A map is OpenMM's:
 * size x size energies in kJ/mol, energy[i + size j] at phi = 2 pi i / size and psi = 2 pi j / size, periodic in both angles, and
 * between the nodes the bicubic patch whose node derivatives come from periodic cubic splines (fx along phi, fy along psi, fxy from
 * the spline of fx along psi: OpenMM's CMAPTorsionForceImpl::calcMapDerivatives).  That is exactly a periodic REMD_CX_TABLE2D block (below) over
 * [0, 2 pi] x [0, 2 pi] with nx = ny = size + 1, the first row and column repeated at the end, and such blocks are what the force
 * carries: consts holds the n_maps blocks back to back and map_offsets[m] is the offset of map m's.  The angles are wrapped by the
 * block's periodic rule.  The force has no program, no per-term parameters and no globals of its own (n_program = 0, n_params = 0,
 * stack_depth ignored; n_globals and global_defaults are the handle's, like every descriptor's).  periodic != 0: every difference inside
 * a dihedral is a minimum image.  Degenerate geometry follows REMD_CX_DIHEDRAL: |b1 x b2|^2 and |b2 x b3|^2 are taken as at least
 * 1e-24 nm^4, so three collinear particles give a finite angle (atan2 of zeros) and finite gradients: the one on the end particle of
 * the collinear triple falls to zero with the cross product, the others keep their formulas.
 * One lane per term, the geometry once, the map picked by index (csrc/cmap.hip); its energy is a column of remd_get_custom_energies
 * and joins the replica's potential; having no globals it adds nothing of its own to the u_kl rows.  remd_set_custom_terms checks the
 * atoms, every map_index and every block's header (nx = ny an integer 3 ... 256, periodic, the range [0, 2 pi], its end inside
 * consts, finite nodes).
 *
 * Donor-acceptor forces (REMD_CUSTOM_HBOND, OpenMM's CustomHbondForce): a donor is up to three particles d1 d2 d3, an acceptor up to
 * three particles a1 a2 a3, and the energy is an expression of the distances, angles and dihedrals among the six (REMD_CX_DISTANCE /
 * REMD_CX_ANGLE / REMD_CX_DIHEDRAL with d1 d2 d3 the particle slots 0 1 2 and a1 a2 a3 the slots 3 4 5; no REMD_CX_VAR: raw coordinates
 * are not variables of this kind), of per-donor and per-acceptor parameters and of global parameters, summed over every (donor,
 * acceptor) pair that no exclusion names and, with a cutoff, whose distance(d1, a1) is below it.  n_terms = hb_n_donors > 0,
 * hb_n_acceptors > 0, atoms NULL, n_params = 0, params NULL, n_particles = 0.  hb_donor_atoms is [hb_n_donors][3] and hb_acceptor_atoms
 * [hb_n_acceptors][3], -1 for a particle the donor or acceptor does not have (the first, d1 / a1, always exists; no particle twice
 * within a row).  hb_particle_mask has bit s set for every particle slot s = 0 ... 5 the program names, and only those: every donor
 * (acceptor) has the particle of every named slot, and the device runs one seeded pass per set bit.  REMD_CX_PARAM operand k is
 * parameter k of the pair's donor for k < hb_n_donor_params (hb_donor_params [hb_n_donors][hb_n_donor_params]), parameter
 * k - hb_n_donor_params of its acceptor behind that (hb_acceptor_params); together at most REMD_CUSTOM_MAX_PARAMS.  Exclusions:
 * hb_excl_offsets [hb_n_donors + 1] and hb_excl_acceptors, donor i is excluded from the acceptors hb_excl_acceptors[hb_excl_offsets[i]
 * ... hb_excl_offsets[i + 1]), each row sorted, no acceptor twice in a row.  A pair that shares a particle must be excluded (refused
 * otherwise).  nb_method and cutoff as for REMD_CUSTOM_NONBONDED: 0 every pair, 1 a cutoff without and 2 with minimum images under the
 * replica's own box (periodic = 1 exactly then: every difference inside a distance, angle or dihedral is then a minimum image, and so
 * is the one of the cutoff test; every box edge must stay >= 2 cutoff, also under a barostat); switch_distance and
 * long_range_correction are ignored.  One wavefront per tile of 64 donors x 64 acceptors, every one of the ceil(nD / 64) ceil(nA / 64)
 * tiles visited (csrc/custom_hbond.hip): the cost is proportional to nD nA, there is no list.  Degenerate geometry follows
 * REMD_CX_DISTANCE / ANGLE / DIHEDRAL.
 *
 * Many-particle forces (REMD_CUSTOM_MANYPARTICLE, OpenMM's CustomManyParticleForce with three particles per set): the energy is an
 * expression of the distances, angles and dihedrals among the particles p1 p2 p3 of a set (REMD_CX_DISTANCE / REMD_CX_ANGLE /
 * REMD_CX_DIHEDRAL with p1 p2 p3 the particle slots 0 1 2; no REMD_CX_VAR), of per-particle parameters and of global parameters,
 * summed over sets of three distinct particles.  n_terms = N, atoms NULL, n_particles = 0, params [N][n_params] with n_params <=
 * REMD_CUSTOM_MAX_PARAMS / 3: REMD_CX_PARAM operand 3 q + s is parameter q of the particle in slot s.  mp_permutation_mode 0
 * (SinglePermutation): every unordered set {i, j, k} once; with a cutoff all three distances must lie below it.  1
 * (UniqueCentralParticle): every set once per choice of its central particle p1, the other two unordered; with a cutoff only the two
 * distances to p1 must lie below it.  A set in which any pair is excluded is skipped (excl_offsets / excl_atoms as for
 * REMD_CUSTOM_NONBONDED, symmetric, and here each row must be sorted and name no particle twice).  mp_types [N] holds every particle's
 * type 0 ... 31; mp_filter[s] has bit t set where type t may fill slot s (all ones: no filter).  Of the assignments of a set to the
 * slots (six in mode 0, the two with p1 the central particle in mode 1) the first in lexicographic order of the atom indices
 * (p1, p2, p3) that passes all three filters is evaluated; a set without one is skipped.  mp_particle_mask has bit s set for every
 * slot the program names, and only those: the device runs one seeded pass per set bit.  nb_method, cutoff and periodic as for
 * REMD_CUSTOM_NONBONDED (switch_distance and long_range_correction are ignored); with nb_method 0 N is at most
 * REMD_CUSTOM_MP_MAX_NEIGHBORS + 1.  Two launches (csrc/custom_manyparticle.hip): a neighbour row of at most
 * REMD_CUSTOM_MP_MAX_NEIGHBORS entries per particle and replica, then one wavefront per central particle over the pairs of its row.
 * A central particle whose row would overflow makes that replica's energy NaN (and adds no force): the device cannot raise, the
 * caller's NaN check sees it, as for the lookup opcodes.  A force evaluation without energies (an MD or minimiser step) drops that
 * particle's sets silently: the NaN appears at the next evaluation with energies.  A particle that cannot be central (mode 1, its type
 * outside mp_filter[0]) is never flagged.
 *
 * Generalized-Born forces (REMD_CUSTOM_GB, OpenMM's CustomGBForce by its definition): up to REMD_CUSTOM_GB_MAX_VALUES computed values
 * per particle and up to REMD_CUSTOM_GB_MAX_TERMS energy terms.  Value 0 is a pair sum, V_0,i = sum over j != i of f(r_ij; i, j) (with
 * a cutoff only r < cutoff counts; excluded j are left out where the stage says so); every later value is an expression of the
 * particle's earlier values and parameters.  An energy term is a sum over particles of an expression of the particle's values and
 * parameters, or a sum over unordered pairs (particle 1 the lower index) of an expression of r and of both particles' values and
 * parameters.  n_terms = N, atoms NULL, n_particles = 0, params [N][n_params], nb_method / cutoff / periodic / excl_offsets / excl_atoms
 * as for REMD_CUSTOM_NONBONDED (symmetric rows).  The force carries no globals of its own: the host folds them into the constants.
 * program holds the programs of all stages back to back and consts their constants; gb_stages is the stage table, gb_n_stages rows of
 * REMD_CUSTOM_GB_STAGE_INTS int32:
 *     [0] type: 0 pair value, 1 single-particle value, 2 single-particle energy term, 3 pair energy term
 *     [1] 1: excluded pairs are left out (pair types)            [2] the value (types 0, 1) or energy term (2, 3) the stage belongs to
 *     [3] pass: an energy term whose expression names more than three differentiated quantities has one stage per pass; its energy
 *         counts in pass 0 only                                  [4] [5] its program: first instruction, instruction count
 *     [6] the stack depth of that program                        [7 ... 9] the quantity that REMD_CX_VAR 0, 1, 2 is; -1: not used
 *     [10] staged columns, 0 ... REMD_CUSTOM_MAX_PARAMS          [11 ... 26] the quantity that REMD_CX_PARAM c is     [27] 0
 * A quantity: 0 = r (pair types); 1 + 2 k + s = value k of particle s; 16 + 2 q + s = parameter q of particle s; s = 0 particle 1 (the
 * particle itself in a single-particle stage, where s = 0 always), 1 particle 2.  The machine differentiates with respect to its three
 * variables, so the quantities to be differentiated (r and the values) are the variables of some pass and staged columns of the
 * others.  Stage 0 is the pair value (variable 0 = r, no value named); the single-particle values follow in order, each naming earlier
 * values only as its variables; the energy stages come last.  Five launches (csrc/custom_gb.hip): the pair value in partial sums per
 * column slice; the values and the single-particle terms with dE/dV; the pair terms (lane i evaluates every pair of its row and keeps
 * half the energy, the dE/dr force on i and dE/dV_k,i); the chain rule back to dE/dV_0; and the chain force sum_j [dE/dV_0,i
 * df(i,j)/dr + dE/dV_0,j df(j,i)/dr].  No lane writes another lane's particle, sums run in a fixed order: results are bit-identical
 * from run to run.  r = 0 between distinct particles gives an energy and no pair force.  The cost is quadratic in N.
 *
 * Tabulated functions (OpenMM's Continuous1DFunction and Discrete1DFunction) of every kind above: REMD_CX_TABLE1D and
 * REMD_CX_LOOKUP1D take one argument x from the stack and push one result; the operand is the offset of the function's block in the
 * force's constants.  The blocks follow the scalar constants, one per function:
 *     REMD_CX_TABLE1D:  [n, min, max, periodic], y[n], y''[n]     (4 + 2 n doubles; n = 2 ... REMD_CUSTOM_MAX_TABLE_POINTS, integral;
 *                                                                  min < max, both finite; periodic 0 or 1)
 *     REMD_CX_LOOKUP1D: [n], values[n]                            (1 + n doubles; n = 1 ... REMD_CUSTOM_MAX_TABLE_POINTS)
 * y are the samples at n uniformly spaced points over [min, max], y'' the second derivatives of the cubic spline through them, solved
 * by the host in f64 (natural: y'' = 0 at both ends; periodic: y''[n-1] = y''[0]).  With h = (max - min) / (n - 1), on interval i,
 * a = (x[i+1] - t) / h, b = (t - x[i]) / h:
 *     y = a y[i] + b y[i+1] + ((a^3 - a) y''[i] + (b^3 - b) y''[i+1]) h^2 / 6,
 *     dy/dt = (y[i+1] - y[i]) / h + ((1 - 3 a^2) y''[i] + (3 b^2 - 1) y''[i+1]) h / 6.
 * (b is computed as (t - min) / h - i and a as 1 - b, so that a + b is exactly 1.)  periodic = 1 wraps the argument,
 * t = x - (max - min) floor((x - min) / (max - min)), clamped into [min, max] (the wrap's rounding may leave it an ulp outside; an
 * argument too large to have a place in the period lands on an end); else t = x.  Out of range: t outside [min, max] (a function that
 * is not periodic) pushes 0 with the derivative 0, OpenMM's reference behaviour; exactly min and max belong to the end intervals; a
 * NaN argument (an infinite one of a periodic function) pushes NaN.  REMD_CX_LOOKUP1D pushes values[round(x)] (halves away from zero, C's round) with the derivative 0, and NaN where the index
 * falls outside 0 ... n - 1: the device cannot raise, and a NaN energy is what a host's NaN check catches.  No argument makes the
 * device load outside the block.  n_consts has no cap of its own: scalars and blocks together, at most what REMD_CUSTOM_MAX_PROGRAM
 * instructions can name (128 one-argument calls of 4 + 2 REMD_CUSTOM_MAX_TABLE_POINTS doubles each, 2 097 664 doubles per force).
 * The long-range correction of a nonbonded force whose expression calls a table is the host's business (openmmtools_amd refuses it).
 *
 *
 * Tabulated functions of two and three arguments (OpenMM's Continuous2DFunction, Discrete2DFunction, Discrete3DFunction):
 * REMD_CX_TABLE2D and REMD_CX_LOOKUP2D take two arguments (x, y) from the stack, first deepest, REMD_CX_LOOKUP3D three (x, y, z); each
 * pushes one result; the operand is the offset of the function's block, which lies among the blocks above:
 *     REMD_CX_TABLE2D:  [nx, ny, xmin, xmax, ymin, ymax, periodic, 0], node[ny][nx][4]   (8 + 4 nx ny doubles; nx, ny integral >= 2;
 *                                                                  min < max, all finite; periodic 0 or 1)
 *     REMD_CX_LOOKUP2D: [nx, ny], values[ny][nx]                  (2 + nx ny doubles; nx, ny integral >= 1)
 *     REMD_CX_LOOKUP3D: [nx, ny, nz, 0], values[nz][ny][nx]       (4 + nx ny nz doubles)
 * with nx ny (nz) <= REMD_CUSTOM_MAX_TABLE_CELLS.  The first index runs fastest: values[i + nx j (+ nx ny k)], OpenMM's order.
 * Node data of REMD_CX_TABLE2D.  The samples f(x_i, y_j) lie on uniform grids over [xmin, xmax] and [ymin, ymax] with spacings hx, hy.
 * Let D be the linear map "samples of a row -> first derivatives at the nodes of the 1D cubic spline through them", the spline of
 * REMD_CX_TABLE1D (natural where periodic = 0, periodic where 1; one flag for both directions): with M its second derivatives,
 *     s'(x_i) = (y[i+1] - y[i]) / h - h (2 M[i] + M[i+1]) / 6,   at the last node (y[n-1] - y[n-2]) / h + h (M[n-2] + 2 M[n-1]) / 6.
 * Every node carries node[j][i] = (f, fx, fy, fxy): fx = D_x f (along x for each j), fy = D_y f (along y for each i), fxy = D_y fx
 * (= D_x fy: the maps act on different indices); the last row and column of a periodic function repeat the first.  A corner is 32
 * contiguous bytes, the two corners of a patch row 64.  The host fits the node data in f64.
 * Evaluation.  In patch (i, j), with u = (x - x_i) / hx computed as (x - xmin) / hx - i and w likewise (the patch index is the integer
 * part, clamped to 0 ... n - 2), the function is the bicubic Hermite interpolant of the four corners (a, b in {0, 1}: corner
 * (i + a, j + b)), with h00(t) = 2 t^3 - 3 t^2 + 1, h01(t) = -2 t^3 + 3 t^2, h10(t) = t^3 - 2 t^2 + t, h11(t) = t^3 - t^2:
 *     F = sum_ab [ h0a(u) h0b(w) f_ab + hx h1a(u) h0b(w) fx_ab + hy h0a(u) h1b(w) fy_ab + hx hy h1a(u) h1b(w) fxy_ab ],
 * dF/dx and dF/dy from the derivatives of the basis divided by hx and hy.  F is C1 across patch edges, interpolates f, reproduces
 * a + b x + c y + d x y, and equals g(x) h(y) of the two 1D splines where the samples are g(x_i) h(y_j).
 * Out of range, per argument by the rules of REMD_CX_TABLE1D: a function that is not periodic pushes 0 with both derivatives 0 where
 * either argument lies outside its range; exactly min and max belong to the end patches; a periodic function wraps each argument,
 * t = x - L floor((x - min) / L), clamped into [min, max]; a NaN argument (an infinite one of a periodic function) pushes NaN,
 * whatever the other argument is.  The lookups push values[round(x) + nx round(y) (+ nx ny round(z))] (C's round) with derivatives 0,
 * and NaN where any index falls outside its range.  No arguments make the device load outside the block.
 *
 * Not provided: Continuous3DFunction, changing a table or a reference after remd_set_custom_terms, pointangle, pointdihedral, interaction
 * groups, collective variables other than the RMSD, a weighted RMSD, energy parameter derivatives of nonbonded, collective-variable and
 * Generalized-Born forces, changing a map or a torsion pair after remd_set_custom_terms.
 *
 * Energy parameter derivatives (OpenMM's addEnergyParameterDerivative / getEnergyParameterDerivatives) of the bond, angle, torsion,
 * external, compound-bond, centroid-bond, donor-acceptor and many-particle kinds: dE/dg of a global column g at the replica's current
 * positions and its own state's globals, in kJ/mol per unit of the parameter.  The machine is a forward-mode differentiator, so the
 * same program gives it exactly: in the derivative mode the REMD_CX_GLOBAL push of column g carries the unit partial, every variable
 * (REMD_CX_VAR, REMD_CX_DISTANCE / ANGLE / DIHEDRAL) is pushed with zero partials, and the result's first partial is dE/dg; piecewise
 * functions differentiate as the branch taken, a lookup's index contributes 0, REMD_CX_POW takes the logarithm term where the exponent
 * varies.  remd_set_custom_parameter_derivatives names the n distinct columns and, per force in the descriptors' order, the mask of
 * those the force declared (bit d: columns[d]); a force contributes to a column only where its bit is set, even if another force's
 * program names the same global (OpenMM's rule).  remd_get_custom_parameter_derivatives evaluates them: one launch per part of the
 * term space that holds a served kind, siblings of the u_kl launches with the same staging (centroids, candidate pairs, neighbour
 * rows), the column loop over the listed derivatives, per-wavefront partials D[r][d][wave] and a fixed-order f64 sum over the
 * wavefronts.  No floating-point atomics: results are bit-identical from run to run and a column's bits do not depend on which other
 * columns are listed.  It runs whatever the states' globals are (also where every state carries the same ones).  A many-particle row
 * over capacity gives NaN in the columns that force declared.  A handle without declared derivatives launches and allocates nothing.
 *
 * remd_get_custom_parameter_derivatives_at_states evaluates the same derivatives under the globals of every state l of
 * remd_set_states (unsampled ones included) at each local replica's current positions: out[r][l][d], what thermodynamic integration
 * and the MBAR expectation of du/dlambda at every state need.  The same launches with a compile-time switch: the staging (centroids,
 * candidate queues, neighbour rows, the particles of a term) runs once per call and the loop over the states sits inside it, the
 * partials are D[r][l][d][wave] in a buffer of R K n (wavefronts) doubles that the first such call allocates, and the same
 * fixed-order sum.  out[r][label_r][d] is bit-identical to remd_get_custom_parameter_derivatives' out[r][d], two states with
 * bit-identical globals give bit-identical results, and a many-particle row over capacity gives NaN at every l.  A handle that never
 * makes the call allocates and launches nothing for it.
 *
 * Global parameters belong to the handle: every force's program addresses the same n_globals columns, and every state carries one
 * value per column (remd_set_custom_globals).  A term acts in every force evaluation (MD steps, energies, the barostat,
 * minimisation); the u_kl rows get beta_l (E_r(g_l) - E_r(g_own(r))) for every state l, E_r(g) the sum of all custom terms at
 * replica r's positions under the globals g.
 *
 * Limits (a descriptor beyond them is refused): REMD_CUSTOM_MAX_PROGRAM instructions per force, REMD_CUSTOM_MAX_STACK stack slots,
 * REMD_CUSTOM_MAX_PARAMS parameters per term, REMD_CUSTOM_MAX_GLOBALS global columns per handle, REMD_CUSTOM_MAX_FORCES forces
 * per handle (of all kinds together), REMD_CUSTOM_MAX_PARTICLES particles per compound bond or groups per centroid bond,
 * REMD_CUSTOM_MAX_TABLE_POINTS points per tabulated function of one argument, REMD_CUSTOM_MAX_TABLE_CELLS values per tabulated
 * function of two or three, REMD_CUSTOM_MAX_CVS collective variables per collective-variable force,
 * REMD_CUSTOM_MAX_MAPS maps per CMAP force (each of at most 255 x 255 energies: (size + 1)^2 <= REMD_CUSTOM_MAX_TABLE_CELLS).
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_CUSTOM_H
#define REMD_HIP_CUSTOM_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_CUSTOM_BOND     0     /* atoms [n][2], variable r                                                              */
#define REMD_CUSTOM_ANGLE    1     /* atoms [n][3], variable theta in [0, pi]                                               */
#define REMD_CUSTOM_TORSION  2     /* atoms [n][4], variable theta in (-pi, pi], the sign convention of PeriodicTorsionForce */
#define REMD_CUSTOM_EXTERNAL 3     /* atoms [n][1], variables x, y, z                                                       */
#define REMD_CUSTOM_COMPOUND 4     /* atoms [n][n_particles], variables x1, y1, z1, ..., and functions of the particles     */
#define REMD_CUSTOM_CENTROID 5     /* atoms [n][n_particles] are GROUP numbers; the particles are the groups' centroids     */
#define REMD_CUSTOM_NONBONDED 6    /* atoms NULL, n_terms = N, params [N][n_params]; variable r of every pair inside the cutoff */

#define REMD_CUSTOM_CV       7     /* atoms NULL, n_terms = 1; variables the RMSDs of the force's collective variables            */

#define REMD_CUSTOM_CMAP     8     /* atoms [n][8] (n_particles = 8): two dihedrals; the energy is map map_index[k] at them; no program */

/* kind 9 is not assigned: a descriptor that carries it is refused as an unknown kind                                              */
#define REMD_CUSTOM_HBOND    10    /* atoms NULL, n_terms = hb_n_donors; functions of the particles d1 d2 d3 a1 a2 a3 of every donor-acceptor pair */

#define REMD_CUSTOM_MANYPARTICLE 11 /* atoms NULL, n_terms = N, params [N][n_params]; functions of the particles p1 p2 p3 of every set of three */

#define REMD_CUSTOM_GB       12    /* atoms NULL, n_terms = N, params [N][n_params]; computed values and energy terms of a CustomGBForce (gb_stages) */

#define REMD_CUSTOM_MAX_PROGRAM 256
#define REMD_CUSTOM_MAX_STACK   16
#define REMD_CUSTOM_MAX_PARAMS  16
#define REMD_CUSTOM_MAX_GLOBALS 16
#define REMD_CUSTOM_MAX_FORCES  8
#define REMD_CUSTOM_MAX_PARTICLES 8
#define REMD_CUSTOM_MAX_CVS   3
#define REMD_CUSTOM_MAX_MAPS  64
#define REMD_CUSTOM_MP_MAX_NEIGHBORS 128     /* the capacity of one particle's neighbour row of a many-particle force          */
#define REMD_CUSTOM_GB_MAX_VALUES 4           /* computed values of a Generalized-Born force                                    */
#define REMD_CUSTOM_GB_MAX_TERMS  8           /* its energy terms                                                               */
#define REMD_CUSTOM_GB_MAX_STAGES 32          /* rows of its stage table: values, and one per energy term and pass              */
#define REMD_CUSTOM_GB_STAGE_INTS 28          /* int32 per row                                                                  */
#define REMD_CUSTOM_MAX_TABLE_POINTS 8192   /* points of one tabulated function of one argument                               */
#define REMD_CUSTOM_MAX_TABLE_CELLS 65536   /* nx ny (nz) of one tabulated function of two or three arguments                  */

/* opcodes */
#define REMD_CX_CONST   0      /* push consts[operand]                                                                      */
#define REMD_CX_VAR     1      /* push variable operand                                                                     */
#define REMD_CX_PARAM   2      /* push the term's parameter operand                                                         */
#define REMD_CX_GLOBAL  3      /* push global column operand at the state in question                                       */
#define REMD_CX_ADD     4
#define REMD_CX_SUB     5
#define REMD_CX_MUL     6
#define REMD_CX_DIV     7
#define REMD_CX_NEG     8
#define REMD_CX_POWI    9      /* a ^ operand, operand a constant integer with |operand| <= 64: multiplications              */
#define REMD_CX_POW     10     /* a ^ b, both from the stack                                                                */
#define REMD_CX_SQRT    11
#define REMD_CX_EXP     12
#define REMD_CX_LOG     13
#define REMD_CX_SIN     14
#define REMD_CX_COS     15
#define REMD_CX_TAN     16
#define REMD_CX_ASIN    17
#define REMD_CX_ACOS    18
#define REMD_CX_ATAN    19
#define REMD_CX_ATAN2   20
#define REMD_CX_SINH    21
#define REMD_CX_COSH    22
#define REMD_CX_TANH    23
#define REMD_CX_ERF     24
#define REMD_CX_ERFC    25
#define REMD_CX_ABS     26
#define REMD_CX_MIN     27
#define REMD_CX_MAX     28
#define REMD_CX_STEP    29     /* 1 for x >= 0, else 0                                                                      */
#define REMD_CX_DELTA   30     /* 1 for x == 0, else 0                                                                      */
#define REMD_CX_SELECT  31     /* select(x, y, z): y where x != 0, else z                                                   */
#define REMD_CX_FLOOR   32
#define REMD_CX_CEIL    33
#define REMD_CX_PERIODICDISTANCE 34   /* (x1, y1, z1, x2, y2, z2): minimum-image distance under the replica's own box        */
#define REMD_CX_DISTANCE 35     /* distance of the particle slots operand & 15, (operand >> 4) & 15; pushes, pops nothing    */
#define REMD_CX_ANGLE    36     /* angle at the middle one of three particle slots, 4 bits each                              */
#define REMD_CX_DIHEDRAL 37     /* dihedral of four particle slots, 4 bits each                                              */
#define REMD_CX_TABLE1D  38     /* the cubic spline of the block at consts[operand] at the argument on the stack               */
#define REMD_CX_LOOKUP1D 39     /* values[round(argument)] of the block at consts[operand]; NaN outside 0 ... n - 1           */
#define REMD_CX_TABLE2D  40     /* the bicubic patch of the block at consts[operand] at the two arguments on the stack          */
#define REMD_CX_LOOKUP2D 41     /* values[round(x) + nx round(y)] of the block at consts[operand]; NaN outside the ranges        */
#define REMD_CX_LOOKUP3D 42     /* values[round(x) + nx round(y) + nx ny round(z)], three arguments; NaN outside the ranges      */
#define REMD_CX_N_OPCODES 43

typedef struct remd_custom_force_desc {
    int32_t kind;                  /* REMD_CUSTOM_*                                                                        */
    int32_t n_terms;               /* bonds / angles / torsions / particles                                                */
    const int32_t* atoms;          /* [n_terms][2 | 3 | 4 | 1 | n_particles]; REMD_CUSTOM_CENTROID: group numbers          */
    int32_t n_params;              /* parameters per term                                                                  */
    const double* params;          /* [n_terms][n_params]                                                                  */
    int32_t n_program;             /* instructions                                                                         */
    const int32_t* program;        /* [n_program][2]: opcode, operand                                                      */
    int32_t n_consts;
    const double* consts;          /* [n_consts]                                                                           */
    int32_t stack_depth;           /* the most stack slots the program holds at once                                       */
    int32_t n_globals;             /* the handle's global-parameter columns: the same in every descriptor of a call        */
    const double* global_defaults; /* [n_globals]: every state's values until remd_set_custom_globals                      */
    int32_t periodic;              /* 1: differences between atoms are minimum images under the replica's own box          */
    int32_t force_group;           /* Force.getForceGroup() (multiple-time-step splittings)                                */
    int32_t n_particles;           /* REMD_CUSTOM_COMPOUND / _CENTROID: particles (groups) per bond, 1 ... REMD_CUSTOM_MAX_PARTICLES; else 0 */
    /* REMD_CUSTOM_CENTROID only (every other kind ignores them)                                                          */
    int32_t n_groups;              /* the force's groups, > 0                                                              */
    const int32_t* group_offsets;  /* [n_groups + 1]: group g holds group_atoms[group_offsets[g] ... group_offsets[g + 1]), none empty */
    const int32_t* group_atoms;    /* atom indices, 0 ... N - 1                                                            */
    const double* group_weights;   /* beside group_atoms: >= 0, summing to 1 in every group (within 1e-12)                 */
    /* REMD_CUSTOM_NONBONDED only (every other kind ignores them)                                                         */
    int32_t nb_method;             /* 0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic                                    */
    double cutoff;                 /* nm (nb_method 1, 2)                                                                  */
    double switch_distance;        /* nm, in (0, cutoff); < 0: no switching function                                       */
    const int32_t* excl_offsets;   /* [N + 1]: particle i is excluded from excl_atoms[excl_offsets[i] ... excl_offsets[i + 1]) */
    const int32_t* excl_atoms;     /* particle indices, symmetric, sorted within a row, never the row's own particle       */
    int32_t long_range_correction; /* 1: the energy gains coeff / V (remd_set_custom_lrc); nb_method 2 only                */
    /* REMD_CUSTOM_CV only (every other kind ignores them)                                                                */
    int32_t n_cvs;                 /* the force's collective variables, 1 ... REMD_CUSTOM_MAX_CVS                          */
    const int32_t* cv_offsets;     /* [n_cvs + 1]: variable k holds cv_atoms[cv_offsets[k] ... cv_offsets[k + 1]), at least 3 */
    const int32_t* cv_atoms;       /* particle indices, 0 ... N - 1, none twice within a variable                          */
    const double* cv_reference;    /* beside cv_atoms, [.][3] nm: each variable's rows centred on their own centroid       */
    /* REMD_CUSTOM_CMAP only (every other kind ignores them)                                                              */
    const int32_t* map_index;      /* [n_terms]: the map of every term, 0 ... n_maps - 1                                   */
    int32_t n_maps;                /* the force's maps, 1 ... REMD_CUSTOM_MAX_MAPS                                         */
    const int32_t* map_offsets;    /* [n_maps]: the offset in consts of each map's block ([nx, ny, 0, 2 pi, 0, 2 pi, 1, 0], node[ny][nx][4]) */
    /* REMD_CUSTOM_HBOND only (every other kind ignores them); it also reads nb_method and cutoff above                   */
    int32_t hb_n_donors;           /* = n_terms, > 0                                                                       */
    int32_t hb_n_acceptors;        /* > 0                                                                                  */
    const int32_t* hb_donor_atoms; /* [hb_n_donors][3]: d1 d2 d3, -1 for an unused second or third particle                */
    const int32_t* hb_acceptor_atoms; /* [hb_n_acceptors][3]: a1 a2 a3, likewise                                           */
    int32_t hb_n_donor_params;     /* per-donor parameters: REMD_CX_PARAM operands 0 ... hb_n_donor_params - 1             */
    const double* hb_donor_params; /* [hb_n_donors][hb_n_donor_params]                                                     */
    int32_t hb_n_acceptor_params;  /* per-acceptor parameters: the operands behind the donor's                             */
    const double* hb_acceptor_params; /* [hb_n_acceptors][hb_n_acceptor_params]                                            */
    const int32_t* hb_excl_offsets; /* [hb_n_donors + 1]: donor i is excluded from hb_excl_acceptors[hb_excl_offsets[i] ... hb_excl_offsets[i + 1]) */
    const int32_t* hb_excl_acceptors; /* acceptor indices, sorted within a row, none twice                                 */
    int32_t hb_particle_mask;      /* bit s: the program names particle slot s (d1 d2 d3 = 0 1 2, a1 a2 a3 = 3 4 5)        */
    /* REMD_CUSTOM_MANYPARTICLE only (every other kind ignores them); it also reads nb_method, cutoff, excl_offsets and excl_atoms above */
    const int32_t* mp_types;       /* [N]: every particle's type, 0 ... 31                                                 */
    int32_t mp_permutation_mode;   /* 0 SinglePermutation, 1 UniqueCentralParticle                                         */
    uint32_t mp_filter[3];         /* per slot p1 p2 p3: bit t set where a particle of type t may fill it (all ones: no filter) */
    int32_t mp_particle_mask;      /* bit s: the program names particle slot s (p1 p2 p3 = 0 1 2)                          */
    /* REMD_CUSTOM_GB only (every other kind ignores them); it also reads nb_method, cutoff, excl_offsets and excl_atoms above */
    const int32_t* gb_stages;      /* [gb_n_stages][REMD_CUSTOM_GB_STAGE_INTS] (the pointer first: it starts at a multiple of 8, where a host that lays the fields out kind by kind puts it) */
    int32_t gb_n_values;           /* computed values, 1 ... REMD_CUSTOM_GB_MAX_VALUES                                     */
    int32_t gb_n_stages;           /* rows of the stage table, 1 ... REMD_CUSTOM_GB_MAX_STAGES                             */
} remd_custom_force_desc;

/* the custom forces of the system; call after remd_set_system (which forgets them).  n = 0: none.  Every custom force of a handle
   sits in one force group.                                                                                                       */
int  remd_set_custom_terms(remd_handle h, const remd_custom_force_desc* desc, int n);
/* values[K][n_globals]: every state's value of each global column; K as in remd_set_states (call after it: the terms refuse to act
   on globals that belong to an older set of states)                                                                              */
int  remd_set_custom_globals(remd_handle h, const double* values);
/* coeff[K][n]: the long-range correction of every state and custom force (kJ/mol nm^3; 0 for a force without one), the descriptors'
   order; call after remd_set_custom_globals (which forgets the coefficients: they are integrals under the globals)               */
int  remd_set_custom_lrc(remd_handle h, const double* coeff);
/* out[R_local][n]: each custom force's energy, in the order of the descriptors whatever their kinds (kJ/mol) at the local replicas' current positions and own states                   */
int  remd_get_custom_energies(remd_handle h, double* out);
/* out[R_local][total]: the RMSD (nm) of every collective variable of the REMD_CUSTOM_CV forces at the local replicas' current
   positions, in the order of the descriptors and of the variables within one (OpenMM's getCollectiveVariableValues)              */
int  remd_get_custom_cv_values(remd_handle h, double* out);
/* the energy parameter derivatives to compute: columns[n] distinct global columns (0 <= n <= REMD_CUSTOM_MAX_GLOBALS; n = 0: none),
   force_masks[number of descriptors]: bit d set where that force declared columns[d].  Call after remd_set_custom_terms (which
   forgets them).  Refused: a column out of range or named twice, a mask bit >= n, a mask bit on a REMD_CUSTOM_NONBONDED, _CV, _CMAP or
   _GB force.                                                                                                                     */
int  remd_set_custom_parameter_derivatives(remd_handle h, const int32_t* columns, int n, const uint32_t* force_masks);
/* out[R_local][n]: dE/d(columns[d]) (kJ/mol per unit of the parameter) summed over the forces that declared it, at the local
   replicas' current positions and own states' globals                                                                           */
int  remd_get_custom_parameter_derivatives(remd_handle h, double* out);
/* out[R_local][K][n]: dE/d(columns[d]) (kJ/mol per unit of the parameter), summed over the forces that declared it, at the local
   replicas' current positions under the globals of state l, for every state l of remd_set_states (unsampled ones included) */
int  remd_get_custom_parameter_derivatives_at_states(remd_handle h, double* out);

#ifdef __cplusplus
}
#endif

#endif
