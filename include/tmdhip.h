/*
 * tmdhip.h — C ABI of the MI355X (gfx950) nonbonded / integrator engine for TorchMD.
 *
 * This is the drop-in boundary of the hot path.  The reference has no native
 * layer at all: its hot path is Python/PyTorch.  Each entry point below therefore cites the
 * reference *Python* function whose arithmetic it replaces; the host-side mirror of the reference
 * API (`torchmd_amd.forces.Forces`, `torchmd_amd.integrator.Integrator`, `torchmd_amd.systems.System`)
 * binds these symbols through ctypes.
 *
 * Conventions
 *   - plain C types only; no torch / C++ types cross the boundary
 *   - `*_dev` pointers are device (HBM) pointers owned by the caller (torch tensors' data_ptr());
 *     `*_host` pointers are host memory, only read during the call
 *   - `real` = float (dtype 0) or double (dtype 1); positions/forces/velocities are [N,3] AoS
 *     contiguous exactly like the reference's `System` tensors (systems.py:12-16)
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream); no call synchronises the device unless documented
 *   - return 0 on success, negative on error; tmdhip_last_error() gives a thread-local message
 *   - one host thread per context (contexts are not re-entrant)
 */
#ifndef TMDHIP_H
#define TMDHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMDHIP_ABI_VERSION 11

/* dtype */
#define TMDHIP_F32 0
#define TMDHIP_F64 1

/* nonbonded term mask — names of reference Forces.nonbonded (forces.py:24) */
#define TMDHIP_TERM_LJ 1u
#define TMDHIP_TERM_ELECTROSTATICS 2u
#define TMDHIP_TERM_REPULSION 4u
#define TMDHIP_TERM_REPULSIONCG 8u

/* layout of the energy accumulator double[TMDHIP_NENERGY] (per replica) */
#define TMDHIP_E_LJ 0
#define TMDHIP_E_ELECTROSTATICS 1
#define TMDHIP_E_REPULSION 2
#define TMDHIP_E_REPULSIONCG 3
#define TMDHIP_E_BONDS 4
#define TMDHIP_E_ANGLES 5
#define TMDHIP_E_DIHEDRALS 6
#define TMDHIP_E_IMPROPERS 7
#define TMDHIP_NENERGY 8

/* compute flags */
#define TMDHIP_WANT_ENERGY 1 /* accumulate (+=) per-term energies into energies_dev          */
#define TMDHIP_WANT_FORCES 2 /* accumulate (+=) forces into forces_dev                        */
#define TMDHIP_COUNT_PAIRS 4 /* also count non-excluded i<j pairs with r <= cutoff (stats)    */
#define TMDHIP_OVERWRITE_FORCES 8 /* store (=) instead of +=: nonbonded, so that the caller need not zero
                                     forces_dev first (the all-pairs path zero-fills internally); bonded
                                     (ABI 4): forces_dev receives the bonded force alone                  */

/* pair-search algorithm */
#define TMDHIP_ALGO_AUTO 0
#define TMDHIP_ALGO_ALLPAIRS 1 /* tiled O(N^2) kernel: small / non-periodic / no-cutoff systems */
#define TMDHIP_ALGO_CELLLIST 2 /* cell binning + Verlet list + list pair kernel                  */

/* switching-force mode (forces.py:403-413) */
#define TMDHIP_SWITCH_REFERENCE 0 /* explicit force = S*f + E*S'/r  (upstream's extra 1/r kept) */
#define TMDHIP_SWITCH_EXACT 1     /* explicit force = S*f + E*S'    (-dE/dr)                      */

typedef struct tmdhip_ctx tmdhip_ctx;

/* Static description of one system's nonbonded interactions.
 * Replaces the state reference `Forces.__init__` derives (forces.py:27-74): the A/B tables
 * (parameters.py:449-457), charges, mapped atom types, and the exclusion set that
 * `_make_indeces` (forces.py:348-357) bakes into its dense pair tensor. */
typedef struct tmdhip_nonbonded_desc {
  int32_t struct_size; /* = sizeof(tmdhip_nonbonded_desc) */
  int32_t dtype;       /* TMDHIP_F32 / TMDHIP_F64: type of pos/forces and of the real-valued arrays below */
  int32_t natoms;
  int32_t ntypes;
  int32_t nreplicas;           /* independent copies of the system (own neighbour lists)  */
  int32_t device;              /* HIP device ordinal                                       */
  const int32_t *types_host;   /* [natoms] index into the A/B tables                       */
  const void *charges_host;    /* real [natoms], units of e                                */
  const void *lj_A_host;       /* real [ntypes*ntypes] or NULL                             */
  const void *lj_B_host;       /* real [ntypes*ntypes] or NULL                             */
  const int32_t *excl_offsets_host; /* CSR [natoms+1]; row i = sorted partners of i (both directions stored) */
  const int32_t *excl_index_host;   /* [excl_offsets[natoms]]                              */
  uint32_t terms;              /* TMDHIP_TERM_* mask                                       */
  int32_t rfa;                 /* reaction field on/off (needs cutoff)                     */
  double cutoff;               /* Angstrom; <= 0: no cutoff                                */
  double switch_dist;          /* Angstrom; <= 0: no switching                             */
  double solvent_dielectric;   /* reference default 78.5                                   */
  int32_t switch_mode;         /* TMDHIP_SWITCH_*                                          */
  int32_t algorithm;           /* TMDHIP_ALGO_*                                            */
  double skin;                 /* Verlet skin in Angstrom; <= 0: library default (1.2)     */
} tmdhip_nonbonded_desc;

/* Bonded topology (already expanded: one parameter row per instance).  Replaces the per-call
 * gathers of forces.py:122-258.  All index arrays are int32 host arrays; params are real. */
typedef struct tmdhip_bonded_desc {
  int32_t struct_size;
  int32_t nbonds;
  const int32_t *bond_idx_host;   /* [nbonds*2]                          */
  const void *bond_prm_host;      /* real [nbonds*2] = (k0, d0)          */
  int32_t nangles;
  const int32_t *angle_idx_host;  /* [nangles*3]                         */
  const void *angle_prm_host;     /* real [nangles*2] = (k0, theta0)     */
  int32_t ndihedrals;             /* distinct proper torsions            */
  const int32_t *dihedral_idx_host;   /* [ndihedrals*4]                  */
  int32_t ndihedral_terms;
  const int32_t *dihedral_term_of_host; /* [nterms] torsion each term belongs to, ascending */
  const void *dihedral_prm_host;        /* real [nterms*3] = (k0, phi0, per)                */
  int32_t nimpropers;
  const int32_t *improper_idx_host;
  int32_t nimproper_terms;
  const int32_t *improper_term_of_host;
  const void *improper_prm_host;
  int32_t n14;
  const int32_t *pair14_idx_host; /* [n14*2]                             */
  const void *pair14_prm_host;    /* real [n14*4] = (A, B, scnb, scee)   */
  uint32_t terms14;               /* TMDHIP_TERM_LJ | TMDHIP_TERM_ELECTROSTATICS: which 1-4 parts are on */
  int32_t bonds_use_cutoff;       /* reference filters bonds by `cutoff` when one is set (forces.py:128-136) */
} tmdhip_bonded_desc;

typedef struct tmdhip_stats {
  int64_t n_compute;        /* tmdhip_compute calls on this replica                         */
  int64_t n_rebuilds;       /* neighbour-list rebuilds                                      */
  int64_t list_entries;     /* entries in the current (full) Verlet list                    */
  int64_t pairs_in_cutoff;  /* result of the last TMDHIP_COUNT_PAIRS call                   */
  int32_t algorithm;        /* algorithm in use                                             */
  int32_t max_neighbours;   /* list capacity per atom                                       */
  int32_t overflow;         /* != 0: a list is currently truncated (see tmdhip_check)       */
  int32_t ncell[3];
  double skin;              /* Verlet skin in use (Angstrom)                                */
  int64_t chains_skipped;   /* MD steps whose rebuild chain the host left out (tmdhip_md_run)  */
  int64_t steps_in_pair_launch; /* MD steps made by step blocks of the pair launch instead of an integrator launch (ABI 4) */
  int64_t fused_step_timeouts;  /* batches rewound because a step block of a fused launch gave up waiting (ABI 5; whole context) */
  int64_t final_steps_in_pair_launch; /* tmdhip_md_run calls whose LAST step (final kick, bonded + kinetic energies) was made by the
                                       * step blocks of the last pair launch (ABI 8; whole context) */
  int64_t batched_launches;     /* pair + step launches that served several replicas of a cell-list context at once (ABI 8; whole context) */
  int64_t pme_evaluations;      /* reciprocal-space (PME) evaluations of this replica (ABI 9)                  */
  int64_t pme_bytes;            /* device memory held by the context's PME buffers and FFT plans (ABI 9)      */
  int64_t charge_by_class;      /* 1: the charges are a function of the LJ class and the lean fp32 pair kernel takes the charge
                                 * products of a pair from its class table; 0: from the gathered records (whole context) */
} tmdhip_stats;

int tmdhip_abi_version(void);
const char *tmdhip_last_error(void);

/* Lifetime.  create copies every host array to the device. */
int tmdhip_create(tmdhip_ctx **out, const tmdhip_nonbonded_desc *desc);
int tmdhip_set_bonded(tmdhip_ctx *ctx, const tmdhip_bonded_desc *desc);
void tmdhip_destroy(tmdhip_ctx *ctx);

/* Smooth particle-mesh Ewald electrostatics (Essmann et al. 1995) for periodic boxes (ABI 9).  With `enable` the
 * electrostatics term of every evaluation becomes the Ewald sum: real space erfc(beta r)/r within the cutoff (pair
 * kernels), reciprocal space on an nx x ny x nz grid with order-`order` cardinal B-splines (pme.hip), the excluded-pair
 * correction -k q_i q_j erf(beta r)/r, the self term -k beta/sqrt(pi) sum q^2 and the neutralising background
 * -k pi Q^2 / (2 V beta^2).  Needs a cutoff, no reaction field, the electrostatics term, order 4..6, grid edges >= order
 * and a non-zero box at compute time.  Creates the FFT plans (rocFFT compiles kernels here, not in the evaluations);
 * synchronises the device.  enable = 0 releases every PME buffer.  Domain decomposition refuses PME contexts. */
typedef struct tmdhip_pme_desc {
  int32_t struct_size; /* = sizeof(tmdhip_pme_desc) */
  int32_t enable;
  double beta;         /* Ewald splitting parameter, 1/Angstrom */
  int32_t grid[3];     /* FFT grid points per box edge */
  int32_t order;       /* B-spline order (4..6) */
} tmdhip_pme_desc;
int tmdhip_set_pme(tmdhip_ctx *ctx, const tmdhip_pme_desc *desc);

/* Holonomic constraints of the MD loop (ABI 10): rigid waters and X-H bond clusters.  tmdhip_md_run then steps every unit —
 * a rigid water, a cluster or an unconstrained atom — in one thread (md_cons.hip: md_step_cons_kernel), in double: after the
 * second half kick the velocity constraint of the unit (its k x k linear system solved exactly), after the drift the position
 * constraint relative to the positions before it (analytic SETTLE for waters, Miyamoto & Kollman 1992; iterated SHAKE for
 * clusters), then v += dx / dt.  The fused pair + step launches, the inline bonded integrator kernel and the replica-batched
 * launch are not used; tmdhip_compute is unaffected (the constrained bond and angle terms stay in the energies).  A cluster
 * that does not converge within max_iter sweeps (or a water too distorted for SETTLE) makes the next tmdhip_md_observe /
 * tmdhip_check return an error.  Copies to the device and synchronises.  enable = 0, or no units, releases everything.
 * Domain decomposition refuses a context with constraints. */
typedef struct tmdhip_constraint_desc {
  int32_t struct_size;               /* = sizeof(tmdhip_constraint_desc) */
  int32_t enable;
  int32_t nwaters;
  int32_t nclusters;
  const int32_t *water_host;         /* [nwaters][3]: O, H1, H2 */
  const double *water_dist_host;     /* [nwaters][2]: d_OH, d_HH (Angstrom) */
  const int32_t *cluster_offsets_host; /* [nclusters + 1]: CSR into cluster_atoms_host (2 .. 5 atoms per cluster) */
  const int32_t *cluster_atoms_host; /* the central atom first, then its hydrogens */
  const double *cluster_dist_host;   /* per entry of cluster_atoms_host: bond length to the central atom (central: unused) */
  double tolerance;                  /* SHAKE: relative bond-length tolerance */
  int32_t max_iter;                  /* SHAKE: sweeps at most */
  int32_t reserved;
} tmdhip_constraint_desc;
int tmdhip_set_constraints(tmdhip_ctx *ctx, const tmdhip_constraint_desc *desc);

/* Virtual interaction sites (added to ABI 11: new symbols only, no existing struct or call changes, so the version constant
 * stays): massless sites at r_s = sum_k w_k r_parent_k with two or three parents and sum_k w_k = 1
 * (the charge site of four-site water: TIP4P-Ew, TIP4P/2005, OPC).  The tables: site [nsites] atom indices, parent [nsites][3]
 * (-1 in the third column: a two-parent site), weight double [nsites][3].  No site is a parent and no two sites share a parent.
 * tmdhip_set_vsites copies them to the device for the context's own launches: in tmdhip_md_run the thread that steps a rigid
 * water (tmdhip_set_constraints) also folds w_k F_site into the three parents' forces before any division by a mass, places the
 * site from the constrained positions as rounded for storage (the expression of tmdhip_vsite_construct), writes its cell-sorted
 * record and runs the Verlet-list displacement test for it; the site's velocity is stored as 0, and when the call returns the
 * forces in forces_dev have been spread (zero site rows).  A site is never a unit of its own: nothing divides by its mass or
 * draws noise for it.  Call it BEFORE tmdhip_set_constraints (which then requires every site's parents to be the O, H1, H2 of
 * one of its waters, in that order, and fails otherwise); with constraints in place it returns an error.  tmdhip_compute* do not
 * look at the tables: a caller of plain evaluations runs the stateless kernels below around them (torchmd_amd.forces does).
 * Copies to the device and synchronises.  enable = 0, or no sites, releases everything. */
typedef struct tmdhip_vsite_desc {
  int32_t struct_size; /* = sizeof(tmdhip_vsite_desc) */
  int32_t enable;
  int32_t nsites;
  int32_t reserved;
  const int32_t *site_host;   /* [nsites] */
  const int32_t *parent_host; /* [nsites][3], -1 = unused (third column only) */
  const double *weight_host;  /* [nsites][3] */
} tmdhip_vsite_desc;
int tmdhip_set_vsites(tmdhip_ctx *ctx, const tmdhip_vsite_desc *desc);

/* Nonbonded block of Forces.compute (forces.py:260-319) for one replica: minimum-image distances
 * (360-372), `dist <= cutoff` filter (76-81), LJ (+switch) / Coulomb / reaction field / repulsion
 * (381-491), force scatter and per-term energy sums (316-319).
 * box_host = the three box edge lengths (diagonal of box[r], forces.py:118); all zero = no wrapping.
 * replica = TMDHIP_ALL_REPLICAS: the body of the reference's `for i in range(nsystems)` loop
 * (forces.py:116) for every replica in one call — pos_dev/forces_dev are the full [R][N][3] arrays,
 * energies_dev is [R][TMDHIP_NENERGY], box_host is [R][3]; all-pairs contexts serve all replicas with
 * one launch per kernel (small systems are launch-bound). */
#define TMDHIP_ALL_REPLICAS (-1)
int tmdhip_compute_nonbonded(tmdhip_ctx *ctx, int replica, const void *pos_dev, const double *box_host,
                             void *forces_dev, double *energies_dev, int flags, void *stream);

/* Bonded block of Forces.compute (forces.py:122-258, 494-605). */
int tmdhip_compute_bonded(tmdhip_ctx *ctx, int replica, const void *pos_dev, const double *box_host,
                          void *forces_dev, double *energies_dev, int flags, void *stream);

/* Forces.compute (forces.py:83-346) for every replica in ONE call with ONE host synchronisation: bonded +
 * nonbonded forces stored into forces_dev (real [R,N,3]; NULL: energies only, `calculateForces=False`) and the
 * per-term energies returned on the host (energies_host: double [R][TMDHIP_NENERGY]).  The neighbour-list
 * validity check rides on the same read-back (for up to 16 replicas one small kernel writes everything into
 * host-mapped memory followed by a sequence word the host spins on; more replicas: copies + stream
 * synchronisation).  Returns 0 = valid; 1 = a list was truncated (capacity grown):
 * call again; negative = error. */
int tmdhip_compute(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev,
                   double *energies_host, void *stream);

/* Synchronises `stream` and verifies that the neighbour lists used since the last check were valid: no
 * device-side rebuild ran out of list capacity.  Returns 0 = results valid; 1 = not valid: the capacity has
 * been grown, the next compute rebuilds, and the caller must repeat the work (a plain evaluation is simply repeated; an
 * MD batch is rewound with tmdhip_md_restore and run again); negative = error. */
int tmdhip_check(tmdhip_ctx *ctx, int replica, void *stream);

/* `niter` iterations of Integrator.step's loop (integrator.py:115-120) for every replica, enqueued from
 * C with no per-step host work:  _first_VV -> Forces.compute (bonded + nonbonded) -> langevin -> _second_VV.
 * Between steps the second half kick of step s-1, the first half step of step s and the neighbour-list
 * displacement test are ONE fused kernel.  Forces of the previous evaluation must be in forces_dev on
 * entry (as the reference requires: run.py:261 primes system.forces); on return forces_dev holds the
 * forces of the last step and velocities have received both half kicks.  (Where the lean fp32 kernel serves the
 * context, the last step — with its energies — is made by the last pair launch itself; energies_dev is complete in
 * stream order when the call returns either way, and a tmdhip_md_observe with TMDHIP_OBSERVE_AFTER_RUN finds the kinetic
 * energy already summed.  Cell-list contexts with several replicas: the pair + step blocks of all replicas share ONE
 * launch per step — ABI 8 —, every replica with its own neighbour state; TMDHIP_BATCH_REPLICAS=0 in the environment
 * keeps the replica-by-replica loop.) */
typedef struct tmdhip_md_desc {
  int32_t struct_size;
  int32_t niter;
  void *pos_dev, *vel_dev, *forces_dev; /* real [R,N,3]                                              */
  const void *mass_dev;                 /* real [N]                                                  */
  const void *vcoeff_dev;               /* real [N] = sqrt(2 gamma kB T dt / m), or NULL: no thermostat */
  const double *box_host;               /* [R*3] box edge lengths                                    */
  double dt;                            /* time step in internal units (fs / 48.88821)               */
  double gamma;                         /* friction in internal units                                */
  uint64_t seed, step0;                 /* noise stream key and position (step0 + iteration)         */
  double *energies_dev;                 /* [R*TMDHIP_NENERGY]: energies of the LAST iteration (overwritten), or NULL */
  int32_t continuation;                 /* != 0: positions and box are what the previous tmdhip_md_run of this context
                                         * left (a hint: the first step may then leave its rebuild chain out like any
                                         * other; a wrong hint costs a rewind, never a wrong result) (ABI 4) */
  int32_t reserved;
} tmdhip_md_desc;
int tmdhip_md_run(tmdhip_ctx *ctx, const tmdhip_md_desc *desc, void *stream);
/* What Integrator.step returns after its loop (integrator.py:121-125), with ONE read-back and ONE host
 * synchronisation: kinetic energy per replica (integrator.py:8-31), the per-term energies of the last step
 * (energies_dev = the buffer given to tmdhip_md_run; NULL: zeros) and the neighbour-list validity check.
 * out_host: double [R][TMDHIP_NENERGY + 1] = per-term energies, then Ekin.  Returns as tmdhip_check.
 * flags (ABI 8): TMDHIP_OBSERVE_AFTER_RUN = the caller vouches that vel_dev / mass_dev are the buffers of the tmdhip_md_run
 * call of this context that has just returned and that NOTHING has written the velocities since (no rescaling, no
 * tmdhip_second_vv, no restore).  Only then may the kinetic energy that the run's last launch has already summed be
 * reused; without the flag (0) the kinetic-energy kernel always runs. */
#define TMDHIP_OBSERVE_AFTER_RUN 1
int tmdhip_md_observe(tmdhip_ctx *ctx, const void *vel_dev, const void *mass_dev, const double *energies_dev,
                      double *out_host, int flags, void *stream);
/* Rewind: copy the state tmdhip_md_run saved at its entry (positions, velocities, forces of every replica)
 * back into desc's buffers.  Used after tmdhip_md_observe / tmdhip_check returned 1 for an MD batch (a list was
 * truncated: the capacity has been grown); the noise stream is counter based, so running the batch again gives
 * the trajectory the truncated run should have produced. */
int tmdhip_md_restore(tmdhip_ctx *ctx, const tmdhip_md_desc *desc, void *stream);

/* Atomic systems only (no exclusions, no bonded terms): replace the atom set of the context — new count,
 * types and charges; the LJ table and all options stay — and mark atoms with index >= nactive (<= 0: none)
 * as passive: they act on the others but get no neighbour list and zero force.  Used by the spatial domain
 * decomposition (a brick's own atoms followed by its halo images) at every atom migration instead of
 * re-creating the context; synchronises the device; the next compute re-plans and rebuilds. */
int tmdhip_update_atoms(tmdhip_ctx *ctx, int natoms, const int32_t *types_host, const void *charges_host,
                        int nactive);

/* Per-atom Verlet skins (cell-list path).  By default every atom may move skin/2 before the list is rebuilt and
 * every pair within cutoff + skin is listed.  With weights w_i in (0, 1] (real [natoms], host) atom i may move
 * s_i = w_i * skin/2 and pair (i, j) is listed within cutoff + s_i + s_j — equally exact (a pair that is not
 * listed cannot come within the cutoff before one of its atoms exceeds its s), but slow atoms (heavy ones: a
 * water oxygen moves 0.28 of what its hydrogens move) stop paying for the skin the fast ones need.  Inside
 * tmdhip_md_run, where velocities are known, a rebuild sizes s_i from the atom's speed as well (0.8 of the static
 * share + the path it covers in 6 fs, at most 1.2 x the largest static share; TMDHIP_VSKIN=0 switches that off).
 * NULL restores the uniform skin.  Synchronises the device; the next compute re-plans and rebuilds. */
int tmdhip_set_skin_weights(tmdhip_ctx *ctx, const void *weights_host);

/* Drop the neighbour list of a replica: the next tmdhip_compute_nonbonded rebuilds it (used after the
 * caller has changed positions out of band, and by the rebuild timing tool). */
int tmdhip_invalidate_list(tmdhip_ctx *ctx, int replica);

/* Host-synchronising query (copies a few words back). */
int tmdhip_get_stats(tmdhip_ctx *ctx, int replica, tmdhip_stats *out);

/* HIP-event timing of the dominant (pair) kernel, recorded on the launch stream.  on = 0: off; low 16 bits = n:
 * every n-th launch (1: every launch); bits 16..27 = stop after that many timed launches (0: no limit); bits 28..30 =
 * launches passed over before the first timed one; bit 31 = launches that also return energies (the last step of a
 * tmdhip_md_run call, tmdhip_compute: another variant of the kernel) are neither timed nor counted.  The
 * start / stop events are attached to the kernel's own dispatch (hipExtLaunchKernel), not recorded around it. */
int tmdhip_timing_enable(tmdhip_ctx *ctx, int on);
int tmdhip_timing_read(tmdhip_ctx *ctx, double *pair_kernel_ms, int64_t *launches, int reset);

/* Integrator kernels (stateless).  n = nreplicas*natoms rows; mass_dev is real [natoms] and is
 * indexed by (row % natoms) exactly like the broadcast of masses [N,1] in integrator.py:61-69. */
/* _first_VV (integrator.py:61-64): pos += vel*dt + 0.5*(F/m)*dt*dt ; vel += 0.5*dt*(F/m) */
int tmdhip_first_vv(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *vel_dev,
                    const void *forces_dev, const void *mass_dev, double dt, void *stream);
/* _second_VV (integrator.py:67-69): vel += 0.5*dt*(F/m) */
int tmdhip_second_vv(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev, const void *forces_dev,
                     const void *mass_dev, double dt, void *stream);
/* langevin (integrator.py:72-74) fused with _second_VV:
 *   vel += -gamma*vel*dt + N(0,1)*vcoeff ; vel += 0.5*dt*(F/m)
 * N(0,1) from a counter-based Philox4x32-10 stream keyed by (seed, step, row). */
int tmdhip_langevin_second_vv(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev,
                              const void *forces_dev, const void *mass_dev, const void *vcoeff_dev,
                              double dt, double gamma, uint64_t seed, uint64_t step, void *stream);
/* kinetic_energy (integrator.py:8-31, batch=None): ke_dev[r] = sum_i 0.5*m_i*|v_ri|^2 (overwrites) */
int tmdhip_kinetic_energy(int dtype, int64_t nreplicas, int64_t natoms, const void *vel_dev,
                          const void *mass_dev, double *ke_dev, void *stream);
/* Wrapper.wrap (wrapper.py:8-30): translate every bonded group by -floor(com/box)*box (com = unweighted
 * mean of its atoms).  pos_dev real [R,N,3] in place; box_dev real [R,3,3] (device, diagonal used; an
 * all-zero box leaves the replica untouched); groups as a CSR over atoms (device int32 arrays; atoms
 * without bonds are groups of one).  has_big_groups != 0 if any group has more than 64 atoms. */
int tmdhip_wrap(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, const void *box_dev, int32_t ngroups,
                const int32_t *group_offsets_dev, const int32_t *group_members_dev, int32_t has_big_groups,
                void *stream);
/* The move of a Monte Carlo barostat (ABI 11): for every replica r and every group g, c = unweighted mean of the
 * group's positions (the centre tmdhip_wrap uses, accumulated in double in both precisions), then every atom of
 * the group is translated by (scale[r] - 1) * c, component by component: the centres follow a box whose edges are
 * multiplied by scale[r], distances inside a group do not change.  A replica whose three factors are exactly 1 is
 * not written.  saved_pos_dev (real [R,N,3], or NULL) receives the positions as they were, from the same launch;
 * restoring a rejected move is a copy from there, never a scaling by 1/s.  scale_host is double [R][3] (read before
 * the call returns).  Groups as for tmdhip_wrap (a CSR that covers every atom once).  Molecules must be whole, not
 * split across the periodic boundary (true of what tmdhip_wrap leaves and of unwrapped trajectories).  Stateless:
 * no context, no atomics, members summed in index order, so two calls on the same input give the same bits. */
int tmdhip_scale_groups(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *saved_pos_dev,
                        const double *scale_host, int32_t ngroups, const int32_t *group_offsets_dev,
                        const int32_t *group_members_dev, int32_t has_big_groups, void *stream);
/* Virtual sites, stateless (added to ABI 11; tables as for tmdhip_set_vsites, but device arrays).  One thread per site, blockIdx.y =
 * replica; arithmetic in double in both precisions, rounded once on the store, parents summed in table order, no atomics: two
 * calls on the same input give the same bits.  Molecules must be whole (as for tmdhip_scale_groups): no minimum image.  A row
 * index outside [0, natoms) makes the kernel skip that site.
 * construct: pos_dev (real [R,N,3]) site rows = sum_k w_k * parent rows.
 * spread:    forces_dev (real [R,N,3]) parent rows += w_k * site row, then the site row is stored as zero. */
int tmdhip_vsite_construct(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, int32_t nsites, const int32_t *site_dev,
                           const int32_t *parent_dev, const double *weight_dev, void *stream);
int tmdhip_vsite_spread(int dtype, int64_t nreplicas, int64_t natoms, void *forces_dev, int32_t nsites, const int32_t *site_dev,
                        const int32_t *parent_dev, const double *weight_dev, void *stream);
/* FIRE energy minimisation, stateless (added to ABI 11): one iteration of every replica from forces that are already in
 * forces_dev.  Bitzek et al., PRL 97, 170201 (2006), with a semi-implicit Euler step on the real masses and a per-atom step cap.
 * state_dev is double [R][2][TMDHIP_FIRE_STATE_DOUBLES]: two slots per replica, each {dt, alpha, npos, done, iterations, fmax,
 * nuphill, 0} (the counters are whole numbers held as doubles).  tmdhip_fire_init writes {dt_start, alpha_start, 0, ...} into
 * both slots.  tmdhip_fire_step reads slot `iteration & 1` and writes the other one, so after k calls with iteration = 0 .. k-1
 * the live slot is k & 1.  partials_dev is scratch, double [R][TMDHIP_FIRE_MAX_BLOCKS][4].
 * For a replica that is not done (all sums over the rows with mass > 0; rows with mass == 0 are neither read nor written):
 *   1. fmax = max_i |F_i|; if fmax < f_tol: done = 1 and nothing moves (`iterations` keeps the number of moves made so far).
 *   2. P = sum F.v, vv = sum v.v, ff = sum F.F.  P > 0: v = (1 - alpha) v + alpha sqrt(vv / ff) F, npos += 1, and if npos > n_min:
 *      dt = min(dt * f_inc, dt_max), alpha *= f_alpha.  Otherwise v = 0, dt *= f_dec, alpha = alpha_start, npos = 0, nuphill += 1.
 *   3. v += dt F / m; if |v_i| dt > max_step: v_i *= (max_step / dt) / |v_i|; x += dt v; iterations += 1.
 * A done replica is never written again.  Two launches (a reduction into per-block partials, an update whose blocks all re-sum
 * the partials in one order), sums and state arithmetic in double in both precisions, no atomics: two runs give the same bits. */
#define TMDHIP_FIRE_STATE_DOUBLES 8
#define TMDHIP_FIRE_MAX_BLOCKS 256
typedef struct tmdhip_fire_params {
  int32_t struct_size; /* = sizeof(tmdhip_fire_params) */
  int32_t n_min;
  double f_tol;    /* force units of forces_dev */
  double dt_start; /* time units in which dt * F / m is a velocity and dt * v a length */
  double dt_max;
  double max_step; /* length: the largest move of one atom in one iteration */
  double f_inc, f_dec, alpha_start, f_alpha;
} tmdhip_fire_params;
int tmdhip_fire_init(int64_t nreplicas, double *state_dev, const tmdhip_fire_params *params, void *stream);
int tmdhip_fire_step(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *vel_dev, const void *forces_dev,
                     const void *mass_dev, double *state_dev, double *partials_dev, const tmdhip_fire_params *params,
                     int64_t iteration, void *stream);
/* Stochastic velocity rescaling (Bussi, Donadio & Parrinello, JCP 126, 014101, 2007) with one target per replica, and
 * centre-of-mass motion removal, stateless (added to ABI 11): one application to velocities that are in vel_dev [R][natoms][3].
 * The per-replica arrays are HOST arrays of nreplicas entries, read before the call returns (they travel as kernel arguments,
 * 16 replicas per pair of launches): kbar = N_f k_B T / 2 (energy units of m v^2), ndof = N_f, c = exp(-dt / tau) in [0, 1],
 * r1 a standard normal, s a chi-squared variate with N_f - 1 degrees of freedom, active (may be NULL: all) != 0 for the
 * replicas to treat.  For an active replica, all sums over the rows with mass > 0 (rows with mass == 0 are neither read nor
 * written):
 *   V_cm = sum m v / sum m if remove_com, else 0;  K = (1/2) sum m v^2 - (1/2) (sum m) V_cm^2;
 *   alpha^2 = c + (1 - c) kbar (r1^2 + s) / (ndof K) + 2 r1 sqrt(c (1 - c) kbar / (ndof K)), alpha = sqrt(max(alpha^2, 0)),
 *   alpha = 1 if K = 0;  v <- alpha (v - V_cm)   (not written at all when c == 1 and remove_com == 0).
 * record_dev is double [R][TMDHIP_THERMOSTAT_RECORD_DOUBLES]: {K_before, alpha, K_after = alpha^2 K, |V_cm|, heat, applications,
 * 0, 0}; `heat` (the sum of K_after - K_before) and `applications` accumulate, so the caller zeroes the record once before the
 * first application.  An inactive replica's velocities and record are not touched.  partials_dev is scratch, double
 * [R][TMDHIP_THERMOSTAT_MAX_BLOCKS][5]; tmdhip_thermostat_workspace returns both sizes in doubles.  Two launches per 16
 * replicas, sums and state arithmetic in double in both precisions, no atomics: two runs give the same bits. */
#define TMDHIP_THERMOSTAT_RECORD_DOUBLES 8
#define TMDHIP_THERMOSTAT_MAX_BLOCKS 256
int tmdhip_thermostat_workspace(int64_t nreplicas, int64_t *record_doubles, int64_t *partials_doubles);
int tmdhip_thermostat_apply(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev, const void *mass_dev,
                            const double *kbar_host, const double *ndof_host, const double *c_host, const double *r1_host,
                            const double *s_host, const int32_t *active_host, int32_t remove_com, double *record_dev,
                            double *partials_dev, void *stream);
/* Velocity rescaling by one given factor per replica, with its energy book-keeping, stateless (added to ABI 11): the device
 * half of temperature replica exchange, where replica slots that trade rungs of a temperature ladder have their velocities in
 * vel_dev [R][natoms][3] scaled by sqrt(T_new / T_old).  factor_host is a HOST array of nreplicas finite factors > 0, read
 * before the call returns (they travel as kernel arguments, 16 replicas per pair of launches).  For every replica, over the
 * rows with mass > 0 (rows with mass == 0 are neither read nor written):
 *   K = (1/2) sum m v^2 (no centre-of-mass term);  v <- factor v, one product in double and one rounding on the store
 *   (not written at all when factor == 1.0: such a replica is reduced and recorded only).
 * record_dev is double [R][TMDHIP_EXCHANGE_RECORD_DOUBLES]: {K_before, factor, K_after = factor^2 K, work, applications};
 * `work` (the sum of K_after - K_before) and `applications` accumulate, so the caller zeroes the record once before the first
 * application.  partials_dev is scratch, double [R][TMDHIP_EXCHANGE_MAX_BLOCKS]; tmdhip_velocity_rescale_workspace returns
 * both sizes in doubles.  Sums and record arithmetic in double in both precisions, no atomics: two runs give the same bits. */
#define TMDHIP_EXCHANGE_RECORD_DOUBLES 5
#define TMDHIP_EXCHANGE_MAX_BLOCKS 256
int tmdhip_velocity_rescale_workspace(int64_t nreplicas, int64_t *record_doubles, int64_t *partials_doubles);
int tmdhip_velocity_rescale(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev, const void *mass_dev,
                            const double *factor_host, double *record_dev, double *partials_dev, void *stream);
/* Harmonic position and distance restraints with one target per replica (added to ABI 11: new symbols only).
 *   position  d = minimum image of (x - x_ref) in the orthorhombic box (no image along an edge of zero); E = k |d|^2 / 2, F = -k d
 *   distance  d = minimum image of (x_i - x_j), r = |d|; E = k (r - r0)^2 / 2 (the bond term with k0 = k / 2),
 *             F_i = -k (r - r0) d / r = -F_j; r = 0: F = 0, E = k r0^2 / 2
 * k >= 0, and k = 0 switches an entry off for that replica.  All real arrays are double HOST arrays, [R] outermost.
 * tmdhip_set_restraints validates, builds one row per restrained atom (its position entry, then its distance entries by
 * restraint index), copies the tables to the device and synchronises; calling it again replaces the tables (how a window's
 * target is moved between two tmdhip_md_run calls); enable = 0, or no entries, releases everything.  Refused: sizes and indices
 * out of range, i == j, two position entries for one atom, negative or non-finite k / r0, non-finite references, a restrained
 * atom that is a virtual site of the context, a context with passive atoms (a brick of the domain decomposition), and, where
 * masses are seen (tmdhip_restraint_apply with velocities, tmdhip_md_run), a restrained atom without mass.  That check reads
 * the masses back once per mass array, told by its address, and again after the set of restrained atoms has changed: the
 * caller must not change the masses of restrained atoms in place afterwards (the kernel leaves the velocity of a row with
 * mass <= 0 alone and never divides by it).
 * With restraints in place tmdhip_md_run integrates under the total force: the restraint force never enters the pair or step
 * kernels; it is applied to the half-step velocities between their launches as the impulse dt a_r(x) / (1 - gamma dt), which
 * the Langevin and half-kick lines of the step turn into exactly the kicks they would have made with a_r inside the force, and
 * after the last step of the call a finishing launch adds dt/2 a_r to the velocities and F_r to forces_dev (the forces the call
 * leaves are total) and sums the restraint energies; tmdhip_md_run fails when 1 - gamma dt <= 0.
 * One thread per restrained atom, arithmetic in double from positions of either dtype, one rounding on each store, rows of
 * atoms in no restraint never written, no floating-point atomics: two runs give the same bits. */
typedef struct tmdhip_restraint_desc {
  int32_t struct_size; /* = sizeof(tmdhip_restraint_desc) */
  int32_t enable;
  int32_t nreplicas;   /* = the context's */
  int32_t npos, ndist;
  int32_t reserved;
  const int32_t *pos_atom_host;  /* [npos] */
  const double *pos_ref_host;    /* [R][npos][3] */
  const double *pos_k_host;      /* [R][npos] */
  const int32_t *dist_pair_host; /* [ndist][2] */
  const double *dist_r0_host;    /* [R][ndist] */
  const double *dist_k_host;     /* [R][ndist] */
} tmdhip_restraint_desc;
int tmdhip_set_restraints(tmdhip_ctx *ctx, const tmdhip_restraint_desc *desc);
/* One evaluation of the context's restraints at pos_dev (real [R][N][3], the context's dtype), box_host [R][3].  Whatever is
 * not NULL is served: forces_dev += F_r; vel_dev += kick F_r / m (needs mass_dev, real [N]); energies_dev (double [R][2]) =
 * (position, distance) energies, overwritten.  A context without restraints: nothing is launched, energies are zeroed. */
int tmdhip_restraint_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                           const void *mass_dev, double kick, double *energies_dev, void *stream);
/* The restraint energies of the last step of the last tmdhip_md_run: out_host double [R][2] = (position, distance).  One small
 * copy and a synchronisation of the stream; zeros without restraints. */
int tmdhip_restraint_energy(tmdhip_ctx *ctx, double *out_host, void *stream);
/* Cross energies for an exchange of windows between replicas: out_host double [R][R][2], entry [i][k] = the (position, distance)
 * energies of replica i's configuration (pos_dev real [R][N][3], box_host [R][3]: row i of each) under row k of the tables the
 * context holds.  tmdhip_restraint_apply's walk with the table row taken from a grid axis of its own: energies only, nothing but
 * a workspace of its own is written (the row tmdhip_restraint_energy reads is left alone), [i][i] has the bits
 * tmdhip_restraint_apply gives for the same state, and two calls give the same bits.  Synchronises the stream.  A context without
 * restraints: nothing is launched, the output is zeroed.  Null arguments are refused before any launch. */
int tmdhip_restraint_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double *out_host, void *stream);
/* Harmonic, optionally flat-bottomed restraints on the distance, angle and dihedral between centres of groups of atoms, with
 * targets, strengths and widths per replica (added to ABI 11: new symbols only).  All in double:
 *   centre    X_g = x_a0 + sum_a w_a mi(x_a - x_a0), a0 the group's first atom, w_a = W_a / sum W (normalised here, the sum in
 *             member order), mi the minimum image d - box rint(d / box) (no image along an edge of zero).  PRECONDITION: every
 *             atom of a group lies within half a box edge of a0 along every periodic axis.
 *   distance  s = |mi(X_a - X_b)|          angle  s = acos(clamp(u.v / |u||v|, -1, 1)), u = mi(X_a - X_b), v = mi(X_c - X_b)
 *   dihedral  s = the torsion of four centres in the convention of the metadynamics CV; delta wrapped into [-pi, pi]
 *   energy    delta = s - s0, u = sign(delta) max(|delta| - flat, 0), E = k u^2 / 2; k = 0 switches an entry off for a replica
 * Singular geometries (r = 0, sin theta = 0, collinear centres of a dihedral) give no force and the energy of the formula.
 * The force on atom a of group g is w_a G_g, G_g the sum of -dE/dX_g over the restraints that name g; an atom in several
 * groups is written by one thread, which adds its memberships by ascending group and, within a group, the restraints by
 * ascending index.  No floating-point atomics: two runs give the same bits.  Rows of atoms in no group are never written.
 * tmdhip_set_group_restraints validates, builds the rows, copies the tables and synchronises; calling it again replaces the
 * tables; enable = 0 or nrestraints = 0 releases everything.  Refused: a wrong struct size or nreplicas, an empty group, an
 * atom twice in one group, an index out of range, a weight that is not finite or not > 0, a restraint that names a group twice
 * or has the wrong number of groups for its kind (kind 0 = distance: 2, 1 = angle: 3, 2 = dihedral: 4; the rest of the row is
 * -1), a negative or non-finite k or flat, a non-finite target, an angle target outside [0, pi], a group atom that is a
 * virtual site of the context, a context with passive atoms and, where masses are seen, a group atom without mass (one
 * read-back per mass array, as for tmdhip_set_restraints).  tmdhip_md_run integrates under the total force as it does with
 * restraints: the impulse dt a(x) / (1 - gamma dt) between launches (two launches: centres, forces) and a finishing launch. */
typedef struct tmdhip_group_restraint_desc {
  int32_t struct_size; /* = sizeof(tmdhip_group_restraint_desc) */
  int32_t enable;
  int32_t nreplicas; /* = the context's */
  int32_t ngroups, nrestraints;
  int32_t reserved;
  const int32_t *group_off_host;    /* [ngroups + 1] */
  const int32_t *member_atom_host;  /* [group_off[ngroups]] */
  const double *member_weight_host; /* raw weights > 0, same length */
  const int32_t *kind_host;         /* [M] */
  const int32_t *groups_host;       /* [M][4], -1 padded */
  const double *target_host;        /* [R][M] */
  const double *k_host;             /* [R][M] */
  const double *flat_host;          /* [R][M] */
} tmdhip_group_restraint_desc;
int tmdhip_set_group_restraints(tmdhip_ctx *ctx, const tmdhip_group_restraint_desc *desc);
/* tmdhip_restraint_apply's contract; energies_dev (double [R][3]) = (distance, angle, dihedral) energies, overwritten. */
int tmdhip_group_restraint_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                                 const void *mass_dev, double kick, double *energies_dev, void *stream);
/* The energies of the last step of the last tmdhip_md_run: out_host double [R][3]; zeros without the term. */
int tmdhip_group_restraint_energy(tmdhip_ctx *ctx, double *out_host, void *stream);
/* Cross energies, tmdhip_restraint_states' contract: out_host double [R][R][3], entry [i][k] = configuration i in box i under
 * row k of the tables; [i][i] has the bits tmdhip_group_restraint_apply gives; the run's energy row is left alone. */
int tmdhip_group_restraint_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double *out_host, void *stream);
/* Generalized-Born implicit solvent, OBC2 (Onufriev, Bashford, Case 2004) with the ACE-type surface-area term, for contexts with
 * open boundaries (added to ABI 11: new symbols only).  Per atom: intrinsic radius r_i (A), descreening scale s_i, and the
 * context's charges.  rho_i = r_i - 0.09, sigma_j = s_j rho_j; every ordered pair i != j counts (bonded pairs too): no minimum
 * image, no cutoff, no exclusions.
 *   I_i = (1/2) sum_j t(r_ij; rho_i, sigma_j), psi = rho_i I_i, B_i = 1 / (1/rho_i - tanh(psi - 0.8 psi^2 + 4.85 psi^3) / r_i)
 *   E_GB = -(k_e/2)(1/eps_in - 1/eps_out) sum_ij q_i q_j / sqrt(r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)))   (i = j included)
 *   E_SA = sum_i 4 pi gamma (r_i + r_probe)^2 (r_i / B_i)^6
 * tmdhip_set_gb validates, uploads and synchronises; enable = 0 releases the state.  Refused before any launch: a null argument
 * or a wrong struct size, a radius <= 0.09 or not finite, a scale < 0, a dielectric constant <= 0, a context with passive atoms,
 * with virtual sites, with PME or with the reaction field (which already stands for the solvent); and by every evaluation, a
 * box with a non-zero edge.
 * With the model in place tmdhip_md_run integrates under the total force exactly as it does with restraints: the impulse
 * dt a(x) / (1 - gamma dt) between launches, and after the last step a finishing launch (dt/2 a to the velocities, F to
 * forces_dev, the energies).  Three pair passes with a per-atom close each; every pair is visited from both sides and every
 * partial sum has one writer: no floating-point atomics, two calls on the same state give the same bits. */
typedef struct tmdhip_gb_desc {
  int32_t struct_size; /* = sizeof(tmdhip_gb_desc) */
  int32_t enable;
  const double *radii_host; /* [N] intrinsic radii, A */
  const double *scale_host; /* [N] descreening scales */
  double solute_dielectric, solvent_dielectric; /* eps_in, eps_out */
  double surface_tension;   /* gamma, kcal/mol/A^2; 0: no surface-area term */
  double probe_radius;      /* A */
} tmdhip_gb_desc;
int tmdhip_set_gb(tmdhip_ctx *ctx, const tmdhip_gb_desc *desc);
/* One evaluation at pos_dev (real [R][N][3], the context's dtype); box_host [R][3] must be all zero.  Whatever is not NULL is
 * served: forces_dev += F; vel_dev += kick F / m (needs mass_dev, real [N]; rows with m <= 0 are left alone); energies_dev
 * (double [R][2]) = (GB, SA), overwritten.  A context without the model: nothing is launched, energies are zeroed. */
int tmdhip_gb_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                    const void *mass_dev, double kick, double *energies_dev, void *stream);
/* The (GB, SA) energies of the last step of the last tmdhip_md_run: out_host double [R][2]; zeros without the model. */
int tmdhip_gb_energy(tmdhip_ctx *ctx, double *out_host, void *stream);
/* The effective Born radii B_i of the last evaluation: out_host double [R][N] (zeros before the first one). */
int tmdhip_gb_born_radii(tmdhip_ctx *ctx, double *out_host);
/* Alchemical decoupling of a solute S from its environment E, one coupling (lambda_vdw, lambda_elec) per replica (added to
 * ABI 11: new symbols only).  The context must have been created with charge 0 and an all-zero Lennard-Jones class for every
 * atom of S, so that its own pair kernels return exactly 0 for the solute; what they leave out is computed here:
 *   cross pairs (i in S, j in E) inside the engine's cutoff (the same minimum image and decision), A, B from the context's table
 *   at the solute's true classes, sigma^6 = A / B:
 *     s = r^6 + alpha sigma^6 (1 - lv);  U_lj = lv (A / s^2 - B / s) sw(r);  U_el = le qq g(r)   (g: plain or reaction field)
 *     dU/dlv = (A / s^2 - B / s) sw - lv (-2 A / s^3 + B / s^2) alpha sigma^6 sw;  dU/dle = qq g(r)
 *   intra: every S-S pair the context's exclusions do not name, at full strength with the context's pair formula, and the
 *   charge part qq / (scee r) of the solute's 1-4 pairs (the bonded kernel reads the context's charges, which are 0).
 * tmdhip_set_alchemical validates, uploads and synchronises; enable = 0 releases the state.  Calling it again moves the
 * couplings.  Refused before any launch: a null argument or a wrong struct size, an index out of range or given twice, a lambda
 * outside [0, 1], a replica with lambda_elec != 0 and lambda_vdw != 1 (the charges have no soft core), alpha < 0, a solute
 * that is not closed under the topology (an exclusion of the context, or a listed bond, angle, torsion or 1-4 pair, that
 * joins S to E), a solute the context counts itself, a cross pair with A > 0 >= B, the repulsion / repulsioncg terms, and a
 * context with PME, the generalized-Born model, virtual sites or passive atoms.
 * With the state in place tmdhip_md_run integrates under the total force as it does with restraints: the impulse
 * dt a(x) / (1 - gamma dt) between launches and a finishing launch (dt/2 a to the velocities, F to forces_dev, the energies).
 * Every force has one writer and every sum a fixed order: no floating-point atomics, two calls give the same bits. */
typedef struct tmdhip_alchemical_desc {
  int32_t struct_size; /* = sizeof(tmdhip_alchemical_desc) */
  int32_t enable;
  int32_t natoms;    /* atoms of the solute */
  int32_t nreplicas; /* = the context's */
  const int32_t *atoms_host;      /* [natoms] indices of the solute */
  const double *charges_host;     /* [natoms] its true charges (e), rounded to the context's dtype */
  const int32_t *classes_host;    /* [natoms] its true Lennard-Jones classes in the context's table */
  const double *lambda_vdw_host;  /* [nreplicas] */
  const double *lambda_elec_host; /* [nreplicas] */
  double alpha;
  int32_t n14;                 /* the solute's 1-4 pairs whose charge part is given back (0: none) */
  int32_t nbonds;              /* topology for the closure check only (NULL: not checked) */
  const int32_t *pair14_host;  /* [n14][2] */
  const double *scee14_host;   /* [n14] */
  const int32_t *bond_idx_host;    /* [nbonds][2] */
  const int32_t *angle_idx_host;   /* [nangles][3] */
  const int32_t *torsion_idx_host; /* [ntorsions][4]: proper and improper */
  int32_t nangles, ntorsions;
} tmdhip_alchemical_desc;
int tmdhip_set_alchemical(tmdhip_ctx *ctx, const tmdhip_alchemical_desc *desc);
/* One evaluation at pos_dev (real [R][N][3]) in the boxes box_host [R][3]: tmdhip_restraint_apply's contract.  Whatever is not
 * NULL is served: forces_dev += F; vel_dev += kick F / m (needs mass_dev; rows with m <= 0 are left alone); energies_dev
 * (double [R][5]) = (cross LJ, cross electrostatics, intra, dU/dlambda_vdw, dU/dlambda_elec), overwritten.  Rows of
 * environment atoms with no solute atom inside the cutoff are not written.  A context without the state: nothing is launched,
 * energies are zeroed. */
int tmdhip_alchemical_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                            const void *mass_dev, double kick, double *energies_dev, void *stream);
/* The five numbers of the last step of the last tmdhip_md_run: out_host double [R][5]; zeros without the state. */
int tmdhip_alchemical_energy(tmdhip_ctx *ctx, double *out_host, void *stream);
/* The cross energy of every replica's configuration at nstates (1 .. 32) other couplings states_host [nstates][2] =
 * (lambda_vdw, lambda_elec), in one pass that shares the distance work: out_host double [R][nstates].  Synchronises the stream. */
int tmdhip_alchemical_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, int32_t nstates, const double *states_host,
                             double *out_host, void *stream);
/* Well-tempered metadynamics on one or two collective variables (added to ABI 11: new symbols only).
 *   CVs       kind 0, distance: r = |minimum image of (x_i - x_j)| (atoms[c][0..1]), not periodic, grid [grid_min, grid_max];
 *             kind 1, dihedral: the torsion of atoms[c][0..3] in radians with the sign of the bonded term, from the
 *             minimum-imaged bond vectors, periodic on [-pi, pi) (grid_min / grid_max are not read)
 *   grid      node k of CV c at lo + k h, h = (hi - lo) / bins; bins + 1 nodes (bins on a periodic CV); a node holds the
 *             analytic sum of the deposited Gaussians and its derivatives, (V, V') or (V, d1 V, d2 V, d1 d2 V), double, the
 *             second CV's index fastest; one grid per replica, or one for all (shared = 1: multiple walkers)
 *   bias      the cubic / bicubic Hermite interpolant of the node values; outside a non-periodic grid the CV is clamped for the
 *             lookup (V constant, no force); F = -dV/ds . ds/dx, the exact derivative of the energy reported
 *   hill      every node += w exp(-sum_c Delta_c^2 / 2 sigma_c^2) and its derivatives (Delta = node - s0, the minimum image on
 *             a periodic CV), no truncation; w = height, or height exp(-V(s0) / kdt) with V(s0) read before the deposition
 * tmdhip_set_metadynamics validates, allocates the zeroed grid(s) and synchronises; calling it again starts from a zeroed grid;
 * enable = 0 releases everything.  Refused: a bad struct size, ncv outside 1..2, an unknown kind, indices out of range, an
 * atom repeated within a CV, non-finite or non-positive sigma, bins < 1, grid_min >= grid_max, a spacing h > sigma / 2, a CV
 * atom that is a virtual site of the context, a context with passive atoms, a wrong nreplicas and, where masses are seen
 * (tmdhip_metad_apply with velocities, tmdhip_md_run), a CV atom without mass (one read-back per mass array, as for restraints).
 * With a bias in place tmdhip_md_run integrates under the total force exactly as it does with restraints: the impulse
 * dt a_b(x) / (1 - gamma dt) on the half-step velocities between the step launches, a finishing launch (dt/2 a_b, forces_dev
 * += F_b, the bias energy and the CVs) after the last step; it fails when 1 - gamma dt <= 0.  The grid is static during a call.
 * One wave per replica, one thread per distinct CV atom, double arithmetic, one rounding on each store, no floating-point
 * atomics anywhere (a deposition has one writer per node; shared walkers add their hills in replica order). */
typedef struct tmdhip_metad_desc {
  int32_t struct_size; /* = sizeof(tmdhip_metad_desc) */
  int32_t enable;
  int32_t nreplicas;   /* = the context's */
  int32_t ncv;         /* 1 or 2 */
  int32_t shared;      /* 0: one grid per replica; 1: one grid, every replica deposits into it */
  int32_t reserved;
  int32_t kind[2];
  int32_t atoms[2][4];
  int32_t bins[2];
  double grid_min[2], grid_max[2], sigma[2];
} tmdhip_metad_desc;
int tmdhip_set_metadynamics(tmdhip_ctx *ctx, const tmdhip_metad_desc *desc);
/* One evaluation of the bias at pos_dev (real [R][N][3], the context's dtype), box_host [R][3].  Whatever is not NULL is
 * served: forces_dev += F_b; vel_dev += kick F_b / m (needs mass_dev, real [N]); out_dev (double [R][3]) = (V, s_0, s_1),
 * overwritten.  A context without metadynamics: nothing is launched, out_dev is zeroed. */
int tmdhip_metad_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                       const void *mass_dev, double kick, double *out_dev, void *stream);
/* One deposition at the CV values of pos_dev, two launches and no synchronisation: log_row_dev (double [R][ncv + 1], a row of
 * the caller's hills log on the device) = (s0..., w) per replica, all heights from the grid as it is, then every node of every
 * grid adds its hill(s).  plain != 0: w = height; otherwise w = height exp(-V(s0) / kdt), kdt = k_B (bias_factor - 1) T. */
int tmdhip_metad_deposit(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double height, double kdt, int plain,
                         double *log_row_dev, void *stream);
/* (V, s_0, s_1) of the last step of the last tmdhip_md_run: out_host double [R][3].  One small copy and a synchronisation of the
 * stream; zeros without metadynamics. */
int tmdhip_metad_energy(tmdhip_ctx *ctx, double *out_host, void *stream);
/* Host copies of the grid(s), for restart and inspection: `count` doubles = grids x nodes x (2 or 4); they synchronise. */
int tmdhip_metad_get_grid(tmdhip_ctx *ctx, double *out_host, int64_t count);
int tmdhip_metad_set_grid(tmdhip_ctx *ctx, const double *in_host, int64_t count);
/* Metadynamics on CVs of groups of atoms (added to ABI 11: new symbols only).  The same grid, interpolant, hills and slot as
 * above (a context holds ONE metadynamics bias, of either flavour; tmdhip_metad_apply / _deposit / _energy / _get_grid /
 * _set_grid and tmdhip_set_metadynamics(enable = 0) serve both), with CVs of any number of atoms (csrc/cv_math.h):
 *   groups    group g = members group_off[g] .. group_off[g + 1] of member_atom / member_weight (distinct atoms, weights finite
 *             and > 0, normalised in member order).  Centre X_g = x_a0 + sum_a w_a mi(x_a - x_a0), a0 the first member, mi the
 *             minimum image: every member must lie within half a box edge of a0 along every periodic axis.
 *   kind 2    group distance   s = |mi(X_A - X_B)|, groups[c][0..1]; not periodic
 *   kind 3    group angle      the angle at X_B of groups[c][0..2] in [0, pi]; not periodic; no force where sin = 0 or an arm is 0
 *   kind 4    group dihedral   the torsion of four centres (the dihedral CV's formula); periodic on [-pi, pi)
 *   kind 5    coordination     s = sum_{i in A} sum_{j in B, j != i} f(r_ij), A, B = groups[c][0..1] (weights not read), r the
 *             minimum-image distance, x = (r - d0) / r0, phi = 1 for x <= 0 and 1 / (1 + x^n) otherwise (x^n by repeated
 *             multiplication); f = phi, or with coord_dmax > 0: (phi - phi_max) / (1 - phi_max) for r < dmax and 0 from dmax on,
 *             phi_max = phi((dmax - d0) / r0).  An atom of both sets is skipped against itself.  Not periodic.
 * A distance or dihedral of single atoms is a kind 2 or 4 of one-atom groups of weight 1.  Refused before any allocation or
 * launch: a bad struct size, a wrong nreplicas, ncv outside 1..2, an unknown kind, null or non-monotonic tables, an empty group,
 * an index out of range or repeated inside a group, a weight that is not finite and > 0, a group index out of range or named
 * twice within one CV, r0 <= 0, n outside 2..24, d0 < 0, dmax <= d0, |A| |B| >= 2^31, sigma / bins / range / spacing as above,
 * a virtual site among the atoms, a context with passive atoms.  Refused where a run or an evaluation starts: a CV atom
 * without mass (where masses are seen), and, with any non-zero box edge, a coordination CV without dmax or with dmax beyond
 * half the shortest non-zero edge.  Two dependent launches per application (centres and pair sums; CVs, bias and the atoms'
 * stores), three per deposition; double arithmetic, one rounding per store, no floating-point atomics, rows of atoms in no CV
 * are never read or written. */
#define TMDHIP_METAD_GROUP_DISTANCE 2
#define TMDHIP_METAD_GROUP_ANGLE 3
#define TMDHIP_METAD_GROUP_DIHEDRAL 4
#define TMDHIP_METAD_COORDINATION 5
typedef struct tmdhip_metad_group_desc {
  int32_t struct_size; /* = sizeof(tmdhip_metad_group_desc) */
  int32_t enable;
  int32_t nreplicas;   /* = the context's */
  int32_t ncv;         /* 1 or 2 */
  int32_t shared;      /* as tmdhip_metad_desc */
  int32_t ngroups;
  int32_t kind[2];
  int32_t groups[2][4]; /* group indices in the CV's order, -1 beyond the kind's number */
  int32_t bins[2];
  int32_t coord_n[2];
  double grid_min[2], grid_max[2], sigma[2];
  double coord_r0[2], coord_d0[2], coord_dmax[2]; /* coord_dmax <= 0: no dmax */
  const int32_t *group_off_host;                  /* [ngroups + 1] */
  const int32_t *member_atom_host;
  const double *member_weight_host;
} tmdhip_metad_group_desc;
int tmdhip_set_metadynamics_groups(tmdhip_ctx *ctx, const tmdhip_metad_group_desc *desc);
/* Instantaneous pressure: the molecular virial (added to ABI 11: new symbols only; the suite pins the number).  For orthorhombic periodic boxes, per replica and axis a:
 *   P_aa V = sum_I M_I V_I,a^2 + W_aa,   P = (P_xx + P_yy + P_zz) / 3
 *   W_aa   = 1/2 sum_i sum_{j in list(i)} d_ij,a f_ij,a - sum_i delta_i,a F_i,a
 * R_I / V_I = the mass-weighted centre of molecule I and its velocity, delta_i = r_i - R_I(i), d_ij the engine's minimum-image
 * vector, f_ij the nonbonded pair force on i as the pair kernels evaluate it (pair_terms: reaction field, plain Coulomb, the
 * real-space Ewald term, LJ with either switching flavour, repulsion, repulsionCG), F_i its sum over i's pairs: the virial of the nonbonded force field under a
 * rigid displacement of whole molecules.  Bonded terms (1-4 included) and constraint forces are intramolecular and appear in
 * neither sum; restraints, the metadynamics bias and external forces are not part of it; there is no long-range dispersion
 * correction (as in the energy).  Molecules must be whole (what tmdhip_wrap leaves, or an unwrapped trajectory): no minimum image
 * inside a molecule.  Every exclusion must lie inside one molecule (the caller checks: torchmd_amd.forces does).
 * tmdhip_set_molecules: the molecules as a CSR over atoms on the host (offsets [nmol + 1], members [natoms]); every atom in
 * exactly one molecule, indices in range, no empty molecule.  Copies to the device and synchronises; calling it again replaces
 * the table.
 * tmdhip_pressure: all replicas.  pos_dev / vel_dev real [R][N][3] (vel_dev NULL: the virial only, the kinetic entries are 0),
 * mass_dev real [N], box_host [R][3], out_host double [R][8] = (sum M V^2 x, y, z; W x, y, z; V; P), energies in kcal/mol
 * (velocities in the integrator's units, as for tmdhip_kinetic_energy), V in A^3, P in kcal/mol/A^3.  On the cell-list path the
 * call advances every replica's list bookkeeping exactly as an evaluation does (displacement test, rebuild chain) and nothing
 * else; it makes separate launches, synchronises the stream once and returns as tmdhip_compute: 0 = valid, 1 = a list was
 * truncated (capacity grown): call again, negative = error.  Refused before any launch: a null argument, a wrong struct size, a
 * box with a zero edge, a context with passive atoms (a brick of the domain decomposition), molecules not set, a molecule
 * whose mass sum is <= 0 (the masses are read back once per mass array).
 * PME contexts (grid and beta fixed, as the barostat scales a PME box): W gains the real-space Ewald branch of pair_terms, the
 * reciprocal part sum_m e(m) [1 - 2 (1 + pi^2 m^2 / beta^2) m_a^2 / m^2] with e(m) the energy of a half-complex mode (Essmann et al.
 * 1995), - sum_i delta_i,a F^rec_i,a and the neutralising background's own value; the self term has no volume dependence and the
 * excluded-pair correction is intramolecular.
 * Sums in double in both precisions, in one fixed order, no floating-point atomics: two calls on the same state give the same
 * bits. */
typedef struct tmdhip_molecule_desc {
  int32_t struct_size; /* = sizeof(tmdhip_molecule_desc) */
  int32_t nmol;
  const int32_t *offsets_host; /* [nmol + 1] */
  const int32_t *members_host; /* [natoms] */
} tmdhip_molecule_desc;
int tmdhip_set_molecules(tmdhip_ctx *ctx, const tmdhip_molecule_desc *desc);
int tmdhip_pressure(tmdhip_ctx *ctx, const void *pos_dev, const void *vel_dev, const void *mass_dev, const double *box_host,
                    double *out_host, void *stream);
/* The move of a virial-driven barostat (stochastic cell rescaling, Berendsen; added to ABI 11): the box edges of replica r are
 * multiplied by scale[r][a] and every molecule follows rigidly: each of its atoms is translated by (s_a - 1) R_a and each velocity
 * by (1 / s_a - 1) V_a, with R = sum m x / sum m and V = sum m v / sum m the MASS-WEIGHTED centre of the molecule and its velocity
 * (the quantities tmdhip_pressure's virial is defined on; tmdhip_scale_groups uses the unweighted mean and leaves velocities).
 * Sums in double in both precisions, members in index order, one rounding on the store.  pos_dev / vel_dev real [R][N][3] in
 * place, mass_dev real [N], scale_host double [R][3] (read before the call returns), the molecules as a CSR over atoms in
 * device int32 arrays (offsets [nmol + 1], members [natoms], every atom once); has_big != 0 if a molecule has more than 64
 * atoms: the launch for those molecules is made only then, so a caller that passes 0 for such a table leaves them where they are
 * while the box changes (the flag is the caller's promise; it is not checked, the table being on the device).  record_dev
 * receives double [R][2] = (K_before, K_after), sum m v^2 / 2 over the atoms before and after the shift (of the
 * velocities as stored); partials_dev is scratch; tmdhip_rescale_molecules_workspace returns both sizes in doubles.  A replica
 * whose three factors are exactly 1 is not written (its record is).  A member of mass 0 (a virtual site) moves with its molecule,
 * its velocity is neither read nor written and it enters no sum; a molecule without mass stays where it is.  Molecules must be
 * whole.  Stateless, no host synchronisation, no floating-point atomics: two calls on the same input give the same bits.
 * Refused before any launch: a bad dtype, bad sizes, a null pointer, a factor that is not positive and finite,
 * pos_dev == vel_dev. */
int tmdhip_rescale_molecules_workspace(int64_t nreplicas, int64_t nmol, int64_t *record_doubles, int64_t *partials_doubles);
int tmdhip_rescale_molecules(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *vel_dev, const void *mass_dev,
                             const double *scale_host, int32_t nmol, const int32_t *offsets_dev, const int32_t *members_dev,
                             int32_t has_big, double *record_dev, double *partials_dev, void *stream);
/* Fill `out_dev` (real [n]) with the N(0,1) stream used by tmdhip_langevin_second_vv (for tests). */
int tmdhip_normal_fill(int dtype, int64_t n, void *out_dev, uint64_t seed, uint64_t step, void *stream);


/* ---- spatial domain decomposition (no reference counterpart: torchmd is single-device) ----
 * One brick = one rank.  pos_dev is the position buffer of the brick's force engine, real [nown + nhalo, 3]:
 * the owned atoms first (integrated in place), then the halo rows the exchange writes.
 *
 * tmdhip_dd_step: on the owned atoms, phases bit 0 = second half kick of the previous step (preceded by the
 * Langevin update when vcoeff_dev != NULL; integrator.py:72-74, 67-69), bit 1 = first half step of this step
 * (integrator.py:61-64); same expressions and rounding as the separate kernels above.  With ref_dev (positions
 * at the last migration, real [nown, 3]) and disp2_dev, phase bit 1 also folds max_i |pos_i - ref_i|^2 into
 * *disp2_dev (float bits, atomic max; the caller zeroes it at a migration). */
int tmdhip_dd_step(int dtype, int64_t nown, void *pos_dev, void *vel_dev, const void *forces_dev,
                   const void *mass_dev, const void *vcoeff_dev, double dt, double gamma, uint64_t seed,
                   uint64_t step, int phases, const void *ref_dev, uint32_t *disp2_dev, void *stream);
/* out_dev[k, :] = pos_dev[index_dev[k], :] + shift_dev[k, :] for the `count` rows of all outgoing halo
 * messages (message order; shift = the periodic image the receiver sees). */
int tmdhip_halo_pack(int dtype, int64_t count, const void *pos_dev, const int32_t *index_dev,
                     const void *shift_dev, void *out_dev, void *stream);

/* Halo-exchange communicator: RCCL point-to-point among the `world` ranks of the brick grid (one process and
 * one GPU per rank).  librccl is opened at run time from `librccl_path` (NULL/"" = default search; pass the copy
 * the process has already mapped, e.g. PyTorch's torch/lib/librccl.so).  Rank 0 draws the id, the caller
 * distributes its TMDHIP_COMM_ID_BYTES bytes to the other ranks by any means (torch.distributed broadcast),
 * every rank then calls tmdhip_comm_create with its HIP device current. */
#define TMDHIP_COMM_ID_BYTES 128
typedef struct tmdhip_comm tmdhip_comm;
int tmdhip_comm_unique_id(const char *librccl_path, void *id_out);
int tmdhip_comm_create(tmdhip_comm **out, const char *librccl_path, const void *id, int rank, int world);
void tmdhip_comm_destroy(tmdhip_comm *comm);
/* The same communicator over an IN-PROCESS transport (ABI 5): all `world` ranks live in one process on one device, one
 * host thread per rank, each with a stream of its own.  An exchange is a rendezvous of the threads around device-side
 * copies ordered by events (no RCCL, no second GPU): what lets tmdhip_dd_run execute at world 2 / 4 / 8 on a one-GPU
 * box with the decisions it takes over RCCL.  Create one hub, then one communicator per rank (any thread); every
 * rank's thread must take part in every exchange (tmdhip_comm_exchange / tmdhip_dd_run); a rank that stays away for
 * 30 s breaks the hub (all later calls fail).  Destroy the communicators before the hub. */
typedef struct tmdhip_local_hub tmdhip_local_hub;
int tmdhip_local_hub_create(tmdhip_local_hub **out, int world);
void tmdhip_local_hub_destroy(tmdhip_local_hub *hub);
int tmdhip_comm_create_local(tmdhip_comm **out, tmdhip_local_hub *hub, int rank);
/* One grouped exchange on `stream`: rows of `width` reals; the first send_counts_host[0] rows of send_dev go to
 * rank 0, the next send_counts_host[1] to rank 1, ...; recv_dev receives recv_counts_host[p] rows from rank p
 * in rank order (the layout of an all-to-all with split sizes, as ncclSend/ncclRecv pairs between the
 * ranks that actually exchange rows — messages to oneself across the periodic boundary included). */
int tmdhip_comm_exchange(tmdhip_comm *comm, int dtype, const void *send_dev, const int64_t *send_counts_host,
                         void *recv_dev, const int64_t *recv_counts_host, int width, void *stream);

/* The step loop of one brick enqueued from C (velocity Verlet + optional Langevin over the decomposed system):
 *   per iteration: tmdhip_dd_step (kick of the previous iteration + drift of this one) -> tmdhip_halo_pack ->
 *   tmdhip_comm_exchange into the halo rows of pos_dev -> nonbonded forces on the owned atoms (ctx: open
 *   boundaries, atoms >= nown passive, see tmdhip_update_atoms);  after the last iteration the owed kick.
 *   (Since ABI 6 the loop runs these as three launches + the exchange per iteration — the update of the owned atoms
 *   with the list's displacement test, their cell-sorted records and their outgoing rows; the same for the halo rows
 *   that arrived; the pair kernel, with the rebuild chain left out while no atom is near its limit — same results
 *   bit for bit; TMDHIP_DD_FUSED=0 in the environment keeps the separate launches.)
 * Every `check_every` iterations the maximum squared displacement since the last migration is max-reduced over
 * the ranks and copied to the host asynchronously; it is examined one check later, so the loop never waits for
 * the device.  When the projected displacement exceeds skin/2 the call returns 1 with *iters_done = the number
 * of complete iterations: the next one has drifted but has neither halo nor forces yet — the caller migrates
 * atoms, evaluates the forces, counts that iteration as done and calls again with first_phases = 3 (a kick is
 * owed; niter may then be 0).  Returns 0 when all niter iterations are done, negative on error.
 * TMDHIP_DD_OVERRUN (2): a displacement that was MEASURED lies beyond skin/2 already — the projection was too
 * optimistic (hot atoms, a large check_every) and halo atoms were missing in the last iterations, so the state is
 * invalid; *iters_done = 0, tmdhip_last_error() says how far the atom went.  Every rank returns it at the same
 * iteration.  The caller goes back to a state it saved at the last migration and repeats with a smaller
 * check_every (torchmd_amd/domain.py does; counter-based noise makes the repeat reproducible). */
#define TMDHIP_DD_OVERRUN 2
typedef struct tmdhip_dd_desc {
  int32_t struct_size;
  int32_t dtype;
  int32_t niter;
  int32_t first_phases;      /* 2: velocities complete on entry; 3: the second half kick of the last step is owed */
  int32_t check_every;       /* iterations between displacement checks                                        */
  int32_t reserved;
  int64_t nown, nhalo;
  void *pos_dev;             /* real [nown + nhalo, 3]                                                        */
  void *vel_dev;             /* real [nown, 3]                                                                */
  void *forces_dev;          /* real [nown + nhalo, 3] (halo rows stay zero)                                  */
  const void *mass_dev;      /* real [nown]                                                                   */
  const void *vcoeff_dev;    /* real [nown] or NULL: no thermostat                                            */
  const void *ref_dev;       /* real [nown, 3]: positions at the last migration                               */
  uint32_t *disp2_dev;       /* running maximum of |pos - ref|^2 (float bits); zero at a migration            */
  double dt, gamma;
  uint64_t seed, step0;      /* noise stream key; iteration i kicks with counter step0 + i                    */
  int64_t nsend;             /* rows of all outgoing messages                                                 */
  const int32_t *send_index_dev;
  const void *send_shift_dev; /* real [nsend, 3]                                                              */
  void *send_buf_dev;        /* real [nsend, 3]                                                               */
  const int64_t *send_counts_host, *recv_counts_host; /* [world] rows per peer; sum(recv) = nhalo             */
  double skin;               /* halo skin: migration when the projected displacement exceeds skin / 2         */
  int64_t since_migration;   /* iterations started since the last migration, on entry                         */
} tmdhip_dd_desc;
int tmdhip_dd_run(tmdhip_ctx *ctx, tmdhip_comm *comm, const tmdhip_dd_desc *desc, int32_t *iters_done,
                  void *stream);
/* Forget the pending displacement read-back (call after every migration). */
int tmdhip_dd_reset(tmdhip_comm *comm);

/* ---- atom migration of a brick, on the device (ABI 6) ----
 * When tmdhip_dd_run returns 1 the caller re-assigns atoms to bricks.  tmdhip_dd_migrate does that for one rank's
 * brick entirely in the library (every rank of the communicator must call it): the brick of every owned atom and
 * the counts per destination, an exchange of the atoms' state rows (id, position in the caller's periodic image,
 * velocity, charge, type, mass) over the communicator, the new owned set in the order of the global ids, the halo
 * plan (which owned atoms each of the 26 neighbour directions sees, with which periodic shift: send_index /
 * send_shift / send_counts in the order tmdhip_dd_run expects), the first halo exchange (positions, charges, types)
 * and the atom set of the force engine `ctx` (what tmdhip_update_atoms does from host arrays; atoms >= nown passive).
 * The arrays are the caller's, with capacities in rows; they are rewritten in place.  All communication happens
 * before anything is overwritten: when a capacity is too small the call returns 2 with need_own / need_rows /
 * need_send set and nothing lost — grow the arrays (their contents need not be kept when need_send == 0: the owned
 * rows are then still in the library's scratch; with need_send > 0 keep the first `nown` rows) and call again with
 * the same struct.  The forces have to be evaluated afterwards (the next tmdhip_compute_nonbonded re-plans the
 * engine's grid and rebuilds its list).  Returns 0, 2 (see above) or a negative error. */
typedef struct tmdhip_dd_brick {
  int32_t struct_size;
  int32_t dtype;
  int32_t rank, world;
  int32_t dims[3];           /* brick grid px, py, pz (rank = (cx py + cy) pz + cz)                           */
  int32_t ntypes_map;        /* entries of type_map_host                                                       */
  double box[3];
  double halo;               /* cutoff + halo skin                                                             */
  int64_t cap_own, cap_rows, cap_send; /* capacities in rows: per-owned-atom arrays, pos_dev, the send list    */
  int64_t nown, nhalo, nsend;          /* in: nown; out: all three                                             */
  int64_t *ids_dev;          /* [cap_own] global atom ids                                                      */
  void *pos_dev;             /* real [cap_rows, 3]: owned rows (wrapped frame), then halo rows                 */
  void *unwrap_dev;          /* real [cap_own, 3]: caller's periodic image - wrapped position                  */
  void *vel_dev;             /* real [cap_own, 3]                                                              */
  void *charge_dev;          /* real [cap_own]                                                                 */
  int32_t *type_dev;         /* [cap_own]                                                                      */
  void *mass_dev;            /* real [cap_own]                                                                 */
  void *ref_dev;             /* real [cap_own, 3]: positions at this migration (tmdhip_dd_desc::ref_dev)       */
  uint32_t *disp2_dev;       /* zeroed                                                                         */
  int32_t *send_index_dev;   /* [cap_send]                                                                     */
  void *send_shift_dev;      /* real [cap_send, 3]                                                             */
  int64_t *send_counts_host, *recv_counts_host; /* [world], written                                            */
  const int32_t *type_map_host; /* [ntypes_map]: atom type -> LJ class of the context, or NULL (identity)      */
  int64_t need_own, need_rows, need_send; /* written on return 2                                               */
} tmdhip_dd_brick;
int tmdhip_dd_migrate(tmdhip_ctx *ctx, tmdhip_comm *comm, tmdhip_dd_brick *brick, void *stream);

/* ---- debug aid (not needed by any caller of the path) ----
 * With TMDHIP_DEBUG_TIMELINE=1 in the environment every block of the list build records {entry cycle, exit cycle,
 * hardware id, longest list | candidates x atoms << 32} (4 x uint64 per block); this copies the last build's records
 * to `out_host` (at most max_bytes) and returns the number of blocks (0: nothing recorded, < 0: error).
 * tools/build_timeline.py. */
int tmdhip_debug_build_timeline(void *out_host, size_t max_bytes);

#ifdef __cplusplus
}
#endif
#endif /* TMDHIP_H */
