/* risvec.h -- C ABI of the MI355X-native vectorised RIS-VEC environment.
 *
 * This is the drop-in boundary for ONE hot path of 20242204033/RIS-VEC-MARL:
 * `Simulation-MARL-BCD/Environment.py` (ENV below) -- class `Environ`, its reset /
 * mobility / geometry / channel-gain / BCD / step() methods.  The reference has no
 * FFI of its own (the boundary there is a Python class, ENV:56); every entry point
 * below names the reference method it replaces, batched over `n_envs` independent
 * environments.  The Python host side (`ris_vec_marl_amd/`) binds these with ctypes;
 * `INTEGRATION.md` shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain C: device pointers, sizes, POD structs.  No torch / HIP types: a stream
 *     is passed as `void*` (a `hipStream_t`; NULL = the default stream).
 *   - All launches are asynchronous on `stream`.  Return value: RISVEC_OK or an
 *     error code; `risvec_last_error()` gives the message (thread-local).
 *   - Arrays are row-major, E = n_envs, V = n_veh, M = n_ris.  Complex arrays are
 *     interleaved (re, im) float pairs.  Every pointer must be 16-byte aligned.
 *   - Random draws: each entry point takes optional "injected draw" arrays (used by
 *     the parity tests, which replay the reference's own MT19937 draws); when NULL
 *     the kernel draws from Philox4x32-10 keyed by (seed; global env id, vehicle,
 *     counter, site), so results do not depend on how envs are sharded over GPUs.
 */
#ifndef RISVEC_H
#define RISVEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RISVEC_ABI_VERSION 17
#define RISVEC_POISSON_TABLE 64   /* entries of the arrival CDF table            */
#define RISVEC_MAX_LANES 8        /* lane coordinates per direction (ref. has 4) */
#define RISVEC_MAX_VEH 64         /* V <= 64: one env's vehicles fit a wavefront */
#define RISVEC_METRICS 16         /* floats per env in `metrics` (14 used)       */
#define RISVEC_PARTNER_SINGLE (-1)      /* alone in a 1-element NOMA group (OMA)     */
#define RISVEC_PARTNER_NONE (-2)        /* in no group / a group of another size     */
#define RISVEC_PARTNER_SECOND (1 << 16) /* added to the index when listed 2nd in pair */

enum {
    RISVEC_OK = 0,
    RISVEC_ERR_ARG = 1,         /* NULL / misaligned pointer, bad struct version    */
    RISVEC_ERR_SHAPE = 2,       /* dimension outside what the kernels support       */
    RISVEC_ERR_LAUNCH = 3,      /* HIP reported a launch error                      */
    RISVEC_ERR_UNSUPPORTED = 4
};

enum { RISVEC_DIR_U = 0, RISVEC_DIR_D = 1, RISVEC_DIR_L = 2, RISVEC_DIR_R = 3 };

/* ENV:70, 263, 311-317 */
enum { RISVEC_CH_FREE = 0, RISVEC_CH_3GPP_UMI = 1, RISVEC_CH_3GPP_UMA = 2, RISVEC_CH_OTHER = 3 };

/* step flags */
enum {
    RISVEC_STEP_METRICS = 1,        /* write metrics[E,16] (the 13 last_* + global_reward) */
    RISVEC_STEP_POWER_W = 2,        /* write power_w[E,2,V]  (last_power_W, ENV:664-666)   */
    RISVEC_STEP_POLICY_ACTION = 4,  /* `action` is the policy output [E,V,2] in [-1,1]; apply
                                       marl_train_bcd.py:1601-1608 in-kernel             */
    RISVEC_STEP_OBS = 8,            /* write obs[E,V,5] (marl_train_bcd.py:819-827)        */
    RISVEC_STEP_REUSE_COLSUM = 16,  /* risvec_step_fused_bcd: c_col is current, skip its rebuild */
    RISVEC_STEP_REUSE_SSUM = 32,    /* risvec_step_fused_bcd: s_sum is current (see RISVEC_BCD_REUSE_SSUM) */
    RISVEC_STEP_REUSE_IDX = 128,    /* risvec_step_fused_bcd: theta_idx is current (see RISVEC_BCD_REUSE_IDX) */
    RISVEC_STEP_THETA_BY_INDEX = 256, /* risvec_step_fused_bcd (with RISVEC_STEP_REUSE_IDX, control_bit = 3, a shape for
                                       which risvec_theta_by_index_supported() is 1): theta is kept BY INDEX -- the sweep
                                       updates state.theta_idx and does not write the complex64 state.theta, the fused
                                       step expands the indices through a 9-entry table.  Same outputs bit for bit;
                                       state.theta is stale until risvec_theta_from_index() materialises it. */
    RISVEC_STEP_STEER = 64,         /* risvec_step_fused: h_r is the steering vector risvec_geometry wrote
                                       (phases_R_i[v,m] = z_v^m, z_v = exp(-j pi angle_v), ENV:249-253): do not
                                       read it; evaluate sum_m theta_m b_m z^m by Horner in float64 from
                                       state.z_r (16 bytes per vehicle instead of 8M).  Only valid while h_r is
                                       what the geometry kernel produced -- not for arbitrary channel draws. */
    RISVEC_STEP_3GPP = 512,         /* risvec_step_kernel() only: the 3GPP member of the form (risvec_step_fused_3gpp*
                                       set it internally; every other step entry point rejects it) */
    RISVEC_STEP_THETA_IDX_CURRENT = 1024, /* risvec_step_fused and the fused form of risvec_step_ring (control_bit = 3,
                                       state.theta_idx given): state.theta_idx holds the candidate index of EVERY element
                                       of state.theta (risvec_random_phase and every sweep that writes the tensor leave
                                       it so), so a kernel may read either.  Never changes the plan or the kernel name
                                       risvec_last_kernel() reports; the byte-bound members then run their by-index
                                       instantiation (1 byte per element instead of 8, same outputs bit for bit): the
                                       software pipeline with or without the non-temporal hint, its ring form, and the
                                       latency-shaped kernels' NT and ALT members.  Every other kernel -- the latency-shaped
                                       members with the default cache policy among them -- ignores the bit.  Unlike
                                       RISVEC_STEP_THETA_BY_INDEX the tensor is not stale. */
    RISVEC_STEP_H_R_STEER_CURRENT = 2048, /* risvec_step_fused and the fused form of risvec_step_ring: state.h_r is exactly
                                       what risvec_geometry wrote from the state.steer_ang / state.z_r now in the state, so
                                       a kernel may rebuild rows instead of reading them.  Like
                                       RISVEC_STEP_THETA_IDX_CURRENT it never changes the plan or the kernel name; where
                                       the plan is the software pipeline (either cache policy, the ring form included)
                                       and n_ris is a multiple of 16, its GEN member runs: the same float64 operations
                                       risvec_geometry used, rounded to the same float32 elements and summed in the same
                                       order -- every output bit for bit, 8 n_ris bytes per vehicle not read
                                       (risvec_last_h_r_rebuilt() tells; the walk stays the pipeline's).  Ignored everywhere else: the latency family,
                                       the generic kernels, n_ris % 16 != 0, steer_ang or z_r NULL.  Not accepted
                                       together with RISVEC_STEP_STEER. */
    RISVEC_STEP_STEER_HEADS_CURRENT = 8192 /* only together with RISVEC_STEP_H_R_STEER_CURRENT (alone: RISVEC_ERR_ARG): the
                                       allocation state.steer_ang points to holds the n_envs * n_veh angles followed AT ONCE
                                       by [n_envs, n_veh, n_ris / 16] complex128 chunk heads, as risvec_steer_heads wrote
                                       them from those angles.  The GEN member then reads the head of each 16-element chunk
                                       (16 bytes) instead of evaluating it with sincospi on every launch and does not read
                                       the angles; the rotations start from the same float64 pair, so every output stays
                                       bit for bit (risvec_last_h_r_heads() tells).  Never changes the plan, the kernel
                                       name or the walk; dropped silently wherever RISVEC_STEP_H_R_STEER_CURRENT is. */
};

/* risvec_bcd flags */
enum {
    RISVEC_BCD_REUSE_COLSUM = 1,   /* caller guarantees c_col matches h_r and b */
    RISVEC_BCD_REUSE_SSUM = 2,     /* caller guarantees theta and c_col are unchanged since the last sweep
                                      wrote s_sum: start from it instead of re-summing theta.c */
    RISVEC_BCD_REUSE_IDX = 4,      /* caller guarantees theta is unchanged since the last sweep wrote theta_idx (the
                                      candidate index of every element): control_bit = 3 then takes the indexed sweep,
                                      which never reads theta (two lanes per env, about a third of the instructions per
                                      coordinate) */
    RISVEC_BCD_NO_THETA = 8        /* with RISVEC_BCD_REUSE_IDX and control_bit = 3: update theta_idx only, leave the
                                      complex64 theta to risvec_theta_from_index() */
};

/* Physics / geometry parameters: the attributes of `Environ` that the driver sets
 * (ENV:57-190, overridden by marl_train_bcd.py:548-779).  Passed by value to kernels. */
typedef struct RisVecParams {
    uint32_t abi_version;       /* = RISVEC_ABI_VERSION                               */
    uint32_t struct_bytes;      /* = sizeof(RisVecParams)                             */
    /* PHY  (ENV:72-77, 125, 555) */
    float bandwidth_mhz;
    float noise_power;
    float p_max;
    float power_scale;
    /* QoS  (ENV:79-82) */
    int32_t qos_enable;
    float r_min_bpshz;
    float d_max_s;
    float qos_penalty;
    /* timing / compute  (ENV:101-116) */
    float time_fast;
    float k_cpu;
    float f_local_max;
    float f_edge_max;
    float cycles_per_bit;
    float cpu_share_floor;      /* raw attribute; the kernels apply ENV:574-577       */
    /* reward  (ENV:138-143, 696-703) */
    float w_d;
    float w_e;
    float reward_clip;
    /* arrivals  (ENV:156, 717-719): rate + its CDF table, built on the host in f64    */
    float arrival_rate;
    float poisson_cdf[RISVEC_POISSON_TABLE];
    /* 3GPP modes  (ENV:186-189, 96) */
    float fc_ghz;
    float shadow_std_los;
    float shadow_std_nlos;
    float rician_k_db;
    float veh_ant_gain;
    int32_t n_lanes;            /* entries used in each lane array (reference: 4)     */
    /* geometry, double: positions are advanced in f64 exactly like the reference     */
    double time_slow;           /* ENV:101 */
    double width, height;       /* ENV:63-64 */
    double lanes_up[RISVEC_MAX_LANES];
    double lanes_down[RISVEC_MAX_LANES];
    double lanes_left[RISVEC_MAX_LANES];
    double lanes_right[RISVEC_MAX_LANES];
} RisVecParams;

/* Device-resident state and outputs of E environments (struct-of-arrays).
 * The struct itself lives in HOST memory; the pointers are device pointers. */
typedef struct RisVecState {
    uint32_t abi_version;
    uint32_t struct_bytes;
    int32_t n_envs, n_veh, n_ris, control_bit;
    int64_t env_offset;     /* global id of local env 0 (multi-GPU sharding; RNG key) */
    /* vehicles (ENV:45-53) */
    double *pos;            /* [E,V,2] f64  x,y                                       */
    int32_t *dir;           /* [E,V]   RISVEC_DIR_*                                   */
    float *vel;             /* [E,V]   m/s (integers)                                 */
    /* geometry (ENV:241-253) */
    float *dist_r;          /* [E,V]   distances_R_i                                  */
    float *ang_r;           /* [E,V]   angles_R_i                                     */
    float *pl;              /* [E,V]   ro^2 / (d_Rv^2.2 d_BR^2.5)   (ENV:270-272)     */
    float *h_r;             /* [E,V,M] c64  phases_R_i                                */
    /* RIS (ENV:171-179) */
    float *theta;           /* [E,M]   c64  elements_phase_shift_complex              */
    const float *b;         /* [M]     c64  phase_R (shared by all envs)              */
    const float *h_d;       /* [E,V]   c64  optional direct link (NULL = 0, as ref.)  */
    float *gain;            /* [E,V]   channel_gains                                  */
    /* queues (ENV:116, 151) */
    float *data_buf;        /* [E,V]   DataBuf, kbit                                  */
    float *mec_q;           /* [E]     mec_queue_cycles                               */
    /* step outputs (ENV:731 + attributes read by the driver) */
    float *rate;            /* [E,V]   vehicle_rate                                   */
    float *data_t;          /* [E,V]                                                  */
    float *data_p;          /* [E,V]                                                  */
    float *reward;          /* [E,V]   per_user_reward                                */
    float *over_power;      /* [E,V]                                                  */
    float *obs;             /* [E,V,5] marl_get_state                                 */
    float *metrics;         /* [E,16]  see RISVEC_METRIC_* (slots 14,15 reserved = 0) */
    float *power_w;         /* [E,2,V] last_power_W (may be NULL unless flag set)     */
    /* BCD cache: c[e,m] = (sum_v h_r[e,v,m]) * b[m] in float64 (pure geometry, like `pl`) */
    double *c_col;          /* c128, ceil(E/64)*64*M elements, LANE-MAJOR: (e,m) at ((e/64)*M+m)*64+e%64;
                               written by risvec_geometry / risvec_colsum, read only by risvec_bcd   */
    double *s_sum;          /* [E]     c128; S = sum_m theta_m c_m left by the last BCD sweep (may be NULL) */
    /* SARL variant only (Simulation-SARL/Environment.py:337-340); the MARL step never writes it */
    float *over_data;       /* [E,V]   (may be NULL for MARL-only use)                 */
    /* steering base z[e,v] = exp(-j pi angle_R[e,v]) in float64 (h_r[e,v,m] = z^m); written by risvec_geometry
       when non-NULL, read by risvec_step_fused with RISVEC_STEP_STEER */
    double *z_r;            /* [E,V]   c128 (may be NULL)                                 */
    /* Candidate index of every theta element as the last sweep left it (0..7 = exp(j 2 pi k / 8), ENV:169, 213;
       8 = the integer 0 of ENV:211, 220), one byte each, row-major [E][32*ceil(M/32)] (rows padded to a multiple of
       32 bytes); written by every control_bit = 3 sweep, read with RISVEC_BCD_REUSE_IDX / RISVEC_STEP_THETA_BY_INDEX
       (may be NULL) */
    uint8_t *theta_idx;
    /* The float64 angle (ENV:248) every h_r row is a function of, written by risvec_geometry next to z_r when non-NULL
       (ang_r is its float32 image): with z_r it is all a kernel needs to rebuild a row bit for bit
       (RISVEC_STEP_H_R_STEER_CURRENT, risvec_h_r_from_steer). */
    double *steer_ang;      /* [E,V]   f64 (may be NULL)                                  */
} RisVecState;

/* Parameters of the single-agent (SARL) environment variant,
 * Simulation-SARL/Environment.py:66-83 (SENV). */
typedef struct RisVecSarlParams {
    uint32_t abi_version;
    uint32_t struct_bytes;
    float time_fast;        /* SENV:67 */
    float bandwidth_mhz;    /* SENV:69 */
    float k_cpu;            /* SENV:70 */
    float cycles_l;         /* SENV:71  L */
    float t_factor1;        /* SENV:80 */
    float t_factor2;        /* SENV:81 */
    float penalty1;         /* SENV:82 */
    float penalty2;         /* SENV:83 */
    float arrival_rate;     /* SENV:78 */
    float poisson_cdf[RISVEC_POISSON_TABLE];
} RisVecSarlParams;

/* metrics slots (ENV line in comment) */
enum {
    RISVEC_METRIC_GLOBAL_REWARD = 0,   /* 721 */
    RISVEC_METRIC_OFF_KBIT_SUM = 1,    /* 612 */
    RISVEC_METRIC_LOCAL_KBIT_SUM = 2,  /* 613 */
    RISVEC_METRIC_MEC_QUEUE = 3,       /* 614 */
    RISVEC_METRIC_BACKLOG_MEAN = 4,    /* 649 */
    RISVEC_METRIC_DELAY_LOCAL = 5,     /* 643 */
    RISVEC_METRIC_DELAY_EDGE_Q = 6,    /* 644 */
    RISVEC_METRIC_DELAY_EDGE_C = 7,    /* 645 */
    RISVEC_METRIC_T_TX = 8,            /* 646 */
    RISVEC_METRIC_MEC_UTIL = 9,        /* 653 */
    RISVEC_METRIC_LOCAL_UTIL = 10,     /* 656 */
    RISVEC_METRIC_QOS_VIOL = 11,       /* 677 */
    RISVEC_METRIC_DELAY = 12,          /* 710 */
    RISVEC_METRIC_ENERGY = 13          /* 711 */
};

typedef void *risvec_stream_t;

uint32_t risvec_abi_version(void);
/* Name of the kernel the calling thread's last risvec_step* / risvec_bcd call dispatched ("" before the first): which
 * member of the fused-step family a shape / batch size takes is a dispatch decision; tests assert it.
 * risvec_colsum and risvec_geometry (when it refreshes c_col) name the column-sum member they launched. */
const char *risvec_last_kernel(void);
/* 1 when the calling thread's last step launch read theta as candidate indices (RISVEC_STEP_THETA_BY_INDEX, or
 * RISVEC_STEP_THETA_IDX_CURRENT where the kernel has that reader), 0 when it read the complex64 state.theta or none. */
int risvec_last_theta_by_index(void);
/* The walk of the calling thread's last software-pipeline launch (k_step_fused_pipe): 0 = its envs front to back, 1 =
 * back to front.  The fused MARL step (ring form included) with the default cache policy alternates the two by the
 * parity of its `counter` argument, so that a launch starts on the lines the launch before read last; the results and
 * the kernel name do not depend on the walk.  Every other pipeline launch (non-temporal, SARL, gain) walks forward. */
int risvec_last_pipe_walk(void);
/* 1 when the calling thread's last step launch rebuilt the h_r rows from state.steer_ang / state.z_r instead of reading
 * them (RISVEC_STEP_H_R_STEER_CURRENT where the plan has a GEN member), else 0. */
int risvec_last_h_r_rebuilt(void);
/* Groups of 64 rows that one wavefront served in the calling thread's last step launch when that launch was a GEN member
 * (risvec_last_h_r_rebuilt() == 1), else 0.  1 = the member without a group loop ran: the launcher picks it exactly when
 * every wavefront owns one group.  Results and kernel name do not depend on it. */
int risvec_last_gen_groups_per_wave(void);
/* 1 when the calling thread's last step launch was a GEN member that read the chunk heads behind state.steer_ang
 * (RISVEC_STEP_STEER_HEADS_CURRENT) instead of evaluating them, else 0. */
int risvec_last_h_r_heads(void);
const char *risvec_last_error(void);

/* Forms of a step call, for risvec_step_kernel(): risvec_step, risvec_step_fused, risvec_step_ring (cached / fused),
 * the T-step launch of risvec_step_fused_multi. */
enum {
    RISVEC_FORM_CACHED = 0,
    RISVEC_FORM_FUSED = 1,
    RISVEC_FORM_CACHED_RING = 2,
    RISVEC_FORM_FUSED_RING = 3,
    RISVEC_FORM_FUSED_MULTI = 4
};
/* Name of the kernel a step call of this `form` with these `flags` would launch for this state's shape and batch size,
 * without launching: the same selector the launchers use, so risvec_last_kernel() after the call returns the same
 * string.  NULL when the form does not exist for the shape (risvec_last_error() says why).  Host-only; reads no
 * device memory. */
const char *risvec_step_kernel(const RisVecState *s, uint32_t flags, int32_t form);

/* FOR TESTS AND SAME-BOX A/Bs ONLY: force a kernel form the dispatch rules would not pick at this size.  Every field
 * is RISVEC_BY_RULE (0) by default: the rules decide.  The forms compute the same bits; only speed differs.  Applies
 * process-wide to later launches; set it from one thread, between launches.  risvec_force_forms(NULL) restores the
 * rules. */
enum { RISVEC_BY_RULE = 0, RISVEC_FORCE_OFF = 1, RISVEC_FORCE_ON = 2 };
typedef struct RisVecForce {
    uint32_t abi_version;       /* = RISVEC_ABI_VERSION                                       */
    uint32_t struct_bytes;      /* = sizeof(RisVecForce)                                      */
    int32_t lat;                /* latency-shaped single step where the shape has a software pipeline: OFF never
                                   (the pipeline), ON at every batch size                     */
    int32_t lat_epw;            /* its envs per wavefront: 0 by rule, or 1 / 2 / 4 (clamped to the shape's members) */
    int32_t lat_nt;             /* its non-temporal form                                      */
    int32_t lat_alt;            /* its alternating walk (taken where the non-temporal form is not) */
    int32_t pipe_nt;            /* non-temporal loads in the software pipeline (MARL, SARL and gain)   */
    int32_t colsum_nt;          /* non-temporal loads in the BCD column sums                  */
    int32_t pipe_rev;           /* the pipeline's walk (fused MARL step, default cache policy): BY_RULE the parity of
                                   the step counter, OFF always forward, ON always backward (the non-temporal form has
                                   no backward kernel and walks forward) */
    int32_t pipe_waves;         /* 0 by rule, else the number of wavefronts the pipeline launches, each with a contiguous
                                   run of env groups: lets a test give one wavefront several groups at a few dozen envs */
} RisVecForce;
int risvec_force_forms(const RisVecForce *f);

/* Fill `p` with the class defaults of ENV:57-190 and the reference driver's lanes
 * (marl_train_bcd.py:446-449).  Host-only helper. */
void risvec_default_params(RisVecParams *p);

/* make_new_game (ENV:733-737) + add_new_vehicles_by_number (ENV:381-410).
 * spawn_ints [E,V,3] int32 = (aux, coord, velocity), buf0 [E] int32 (the single
 * randint(5,9) of ENV:737); both NULL -> Philox.  Writes pos, dir, vel, data_buf.
 * Like the reference it does NOT touch mec_q, theta, gain. */
int risvec_reset(const RisVecState *s, const RisVecParams *p, const int32_t *spawn_ints,
                 const int32_t *buf0, uint64_t seed, uint32_t counter, risvec_stream_t stream);

/* renew_positions (ENV:412-542).  u_turn [E,V,8] float32 uniform draws consumed left
 * to right, one per detected lane crossing; NULL -> Philox.  n_used [E,V] int32
 * (optional) receives the number of draws consumed.  A move may need 2 * n_lanes draws (one per lane of the two
 * lists a direction looks at); a u_turn row and the two Philox sites hold 8, so p->n_lanes > 4 is refused with
 * RISVEC_ERR_UNSUPPORTED. */
int risvec_mobility(const RisVecState *s, const RisVecParams *p, const float *u_turn,
                    int32_t *n_used, uint64_t seed, uint32_t counter, risvec_stream_t stream);

/* compute_parms (ENV:241-253): pos -> dist_r, ang_r, pl, h_r. */
int risvec_geometry(const RisVecState *s, const RisVecParams *p, risvec_stream_t stream);

/* The h_r rows as the GEN members of the fused step rebuild them: out [E,V,M] c64 (16-byte aligned) from
 * state.steer_ang / state.z_r, by the routine risvec_geometry itself runs.  n_ris must be a multiple of 16.  After
 * risvec_geometry, `out` equals state.h_r bit for bit; tests compare the two. */
int risvec_h_r_from_steer(const RisVecState *s, float *out, risvec_stream_t stream);

/* The head of every 16-element chunk of every h_r row in float64: heads[e,v,c] = exp(-j pi steer_ang[e,v] 16 c) as
 * (re, im), [E,V,M/16] complex128 (16-byte aligned), by the routine risvec_geometry starts each chunk with.  n_ris must
 * be a multiple of 16.  The heads are a function of state.steer_ang alone: write them after risvec_geometry, directly
 * behind the angles, and the fused step may be sent RISVEC_STEP_STEER_HEADS_CURRENT until the angles change. */
int risvec_steer_heads(const RisVecState *s, double *heads, risvec_stream_t stream);

/* update_channel_gains, "free" model (ENV:263-273): theta, h_r, b, pl -> gain. */
int risvec_gain(const RisVecState *s, const RisVecParams *p, risvec_stream_t stream);

/* update_channel_gains, 3GPP modes (ENV:275-327).  model = RISVEC_CH_*.  Injected
 * draws (all [E,V] float32, all or none): u_los ~ U[0,1), z_shadow ~ N(0,1),
 * small = small-scale power (ENV:13-25).  NULL -> Philox (Rayleigh or Rice per
 * p->rician_k_db). */
int risvec_gain_3gpp(const RisVecState *s, const RisVecParams *p, int32_t model,
                     const float *u_los, const float *z_shadow, const float *small,
                     uint64_t seed, uint32_t counter, risvec_stream_t stream);

/* Column sums for BCD: c_col[e,m] = (sum_v h_r[e,v,m]) * b[m], float64.  One HBM pass over
 * h_r.  risvec_geometry calls it too, so after compute_parms the cache is current; call it
 * again after writing h_r directly. */
int risvec_colsum(const RisVecState *s, risvec_stream_t stream);

/* optimize_phase_shift (ENV:208-220) with the objective of ENV:222-231: one BCD sweep
 * over theta in place.  Rebuilds c_col first unless flags has RISVEC_BCD_REUSE_COLSUM.
 * idx_out [E,M] int32 (optional): chosen candidate, -1 = none. */
int risvec_bcd(const RisVecState *s, const RisVecParams *p, int32_t *idx_out, uint32_t flags,
               risvec_stream_t stream);

/* get_next_phase (ENV:233-239): theta = exp(j*angle), angle [E,M] float32. */
/* state.theta[e,m] = the complex64 image of candidate state.theta_idx[e,m]: materialises theta after sweeps that kept
 * it by index (RISVEC_BCD_NO_THETA / RISVEC_STEP_THETA_BY_INDEX).  What those sweeps would have stored, bit for bit. */
int risvec_theta_from_index(const RisVecState *s, risvec_stream_t stream);
/* 1 when the fused step has a theta-by-index form for this shape (RISVEC_STEP_THETA_BY_INDEX), else 0 */
int risvec_theta_by_index_supported(int32_t n_veh, int32_t n_ris);

int risvec_set_phase(const RisVecState *s, const float *angle, risvec_stream_t stream);

/* Random_phase (ENV:203-206): theta = exp(j*possible_angles[idx]); idx [E,M] int32 or
 * NULL -> Philox.  With control_bit = 3 and state.theta_idx given, the candidate index of every element is written
 * there too. */
int risvec_random_phase(const RisVecState *s, const int32_t *idx, uint64_t seed,
                        uint32_t counter, risvec_stream_t stream);

/* step (ENV:547-731) with compute_data_rate (ENV:331-372), using the cached `gain`.
 * action [E,2,V] float32 (or [E,V,2] policy output with RISVEC_STEP_POLICY_ACTION),
 * partner [E,V] int32 + n_groups [E] int32 encode `noma_groups`, arrivals [E,V] int32
 * = the Poisson draws of ENV:718 (NULL -> Philox, counter = step index). */
int risvec_step(const RisVecState *s, const RisVecParams *p, const float *action,
                const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals,
                uint64_t seed, uint32_t counter, uint32_t flags, risvec_stream_t stream);

/* compute_data_rate (ENV:331-372) on its own: p_off [E,V] float32 = offload power in W
 * (row 0 of the reference's `power`), cached `gain` -> rate_out [E,V] bit/s/Hz. */
int risvec_data_rate(const RisVecState *s, const RisVecParams *p, const float *p_off,
                     const int32_t *partner, const int32_t *n_groups, float *rate_out,
                     risvec_stream_t stream);

/* The fused north-star kernel: update_channel_gains ("free") + step in ONE launch:
 * one HBM pass over h_r and theta, gains exchanged in LDS, also written to `gain`. */
int risvec_step_fused(const RisVecState *s, const RisVecParams *p, const float *action,
                      const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals,
                      uint64_t seed, uint32_t counter, uint32_t flags, risvec_stream_t stream);

/* Trajectory record of a multi-step launch: what the driver reads after every step (per-user rewards
 * TRAIN:1611, the observation TRAIN:819-827, the metrics row TRAIN:1627-1662), one slice per step.
 * Device pointers; any of them may be NULL (not recorded). */
typedef struct RisVecTraj {
    float *reward;          /* [T,E,V]                                                 */
    float *obs;             /* [T,E,V,5]                                               */
    float *metrics;         /* [T,E,16]                                                */
} RisVecTraj;

/* The T-step launch: exactly `n_steps` consecutive risvec_step_fused calls -- the driver's step loop
 * marl_train_bcd.py:1304-1611 between two channel refreshes, with the NOMA groups frozen as they are inside an
 * episode -- in ONE launch.  actions [T,E,2,V] (or [T,E,V,2] with RISVEC_STEP_POLICY_ACTION); arrivals [T,E,V]
 * int32 or NULL (Philox, counter + t at step t, i.e. the counters T single calls would use); partner /
 * n_groups are the same for every step.  The state tensors end up exactly as after the last of the T single calls
 * (bit for bit); every step's reward / obs / metrics additionally go to traj (may be NULL).  h_r and theta
 * cannot change inside the launch, so the cascaded gains are computed once and each env's queues stay in
 * registers: at small batches (BASELINE configs[1]) this removes the per-step launch and memory round trip
 * that bound a single-step launch.  RISVEC_STEP_REUSE_* / RISVEC_STEP_STEER are not accepted here. */
int risvec_step_fused_multi(const RisVecState *s, const RisVecParams *p, int32_t n_steps, const float *actions,
                            const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals,
                            uint64_t seed, uint32_t counter, uint32_t flags, const RisVecTraj *traj,
                            risvec_stream_t stream);

/* The same on the CACHED gains (state.gain as risvec_gain / a fused step left it): exactly `n_steps` consecutive
 * risvec_step calls in one launch, for any shape -- the reference driver's own cadence, step() every step and the
 * channel gains only every K_STEPS_FOR_RIS_OPTIMIZATION = 100 steps (marl_train_bcd.py:1304-1611, 1307-1309).
 * Arguments as risvec_step_fused_multi; h_r / theta are not read. */
int risvec_step_multi(const RisVecState *s, const RisVecParams *p, int32_t n_steps, const float *actions,
                      const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals,
                      uint64_t seed, uint32_t counter, uint32_t flags, const RisVecTraj *traj,
                      risvec_stream_t stream);

/* SARL variant: Simulation-SARL/Environment.py step(action_power, action_phase)
 * SENV:321-359 for every env: get_next_phase (theta = exp(j*action_phase), action_phase [E,M]
 * float32 radians; NULL keeps the current theta), the RIS cascaded gain, natural-log rate against
 * sigma^2 = 1e-14, cube-root local-CPU model, buffer-length reward with its two penalties,
 * Poisson arrivals.  action_power [E,2,V] is used as given (no projection).  Outputs: data_buf,
 * data_t, data_p, over_power, over_data, rate, reward [E,V] and the mean reward in
 * metrics[e,0]; with RISVEC_STEP_OBS also obs[E,V,5] = the non-theta tail of ddpg_train.py:47-73. */
int risvec_sarl_step(const RisVecState *s, const RisVecSarlParams *p, const float *action_power,
                     const float *action_phase, const int32_t *arrivals, uint64_t seed,
                     uint32_t counter, uint32_t flags, risvec_stream_t stream);

/* The SARL rollout step in ONE launch (Simulation-SARL ddpg_train.py:114-185 between the actor's output and the replay
 * buffer), per env with A = 2 n_veh + n_ris:
 *   1. OU exploration noise (noise.py:12-17): x' = x + ou_theta (ou_mu - x) ou_dt + ou_sigma sqrt(ou_dt) z on ou_x [E,A]
 *      in place; z [E,A] ~ N(0,1) injected, or NULL: Philox4x32-10 at (ou_env_offset + e, j, counter, site 11; ou_seed)
 *      for the element PAIR j, Box-Muller of its words (.x, .y) giving elements 2j and 2j + 1.  ou_x NULL: no noise.
 *   2. a = clamp(mu + x', -0.999, 0.999) -> action [E,A] (ddpg_torch.py:42, ddpg_train.py:151): the stored action row.
 *   3. power p0_v = (a_v + 1)/2, p1_v = (a_{V+v} + 1)/2; phase_m = ((a_{2V+m} + 1)/2) 2 pi -> phase [E,M] (:154-158).
 *   4. get_next_phase: theta = exp(j phase) -> state.theta, bit for bit what risvec_set_phase stores; the cascade reads
 *      it on chip.
 *   5. the cascaded gains and step() of risvec_sarl_step (RISVEC_STEP_OBS implied: state.obs receives the 5-float tail).
 *   6. obs_full [E, V, M/V + 5]: agent v's slice phase[v tn : (v+1) tn], tn = M / V, then the tail (ddpg_train.py:47-73).
 *   7. with the ring pointers set (all five, or none): row (mem_cntr + e) % mem_size receives state = obs_full as the
 *      kernel found it, action = a, reward = metrics[e,0], new_state = the new obs_full, terminal = done (buffer.py:13-21).
 *      The caller advances its mem_cntr by n_envs.
 * Shapes: n_veh in {4, 8, 16}, even n_ris with n_veh <= n_ris <= 256 (risvec_sarl_rollout_supported); others return
 * RISVEC_ERR_UNSUPPORTED: use the staged path (risvec_sarl_step after mapping the action on the host side). */
typedef struct RisVecSarlRollout {
    uint32_t struct_bytes;      /* = sizeof(RisVecSarlRollout)                           */
    int32_t done;               /* terminal flag of this step's transitions              */
    const float *mu;            /* [E,A]   raw actor output, read in place               */
    float *ou_x;                /* [E,A]   OU state, updated in place (NULL: no noise)   */
    const float *z;             /* [E,A]   injected N(0,1) draws (NULL: Philox)          */
    float ou_theta, ou_mu, ou_sigma, ou_dt;
    uint64_t ou_seed;           /* Philox key and global id of local env 0 for the noise */
    int64_t ou_env_offset;
    float *action;              /* [E,A]                                                 */
    float *phase;               /* [E,M]   elements_phase_shift_real                     */
    float *obs_full;            /* [E,V,M/V+5] read (ring `state`) and rewritten         */
    float *state_memory;        /* [mem_size, V (M/V+5)]                                 */
    float *action_memory;       /* [mem_size, A]                                         */
    float *reward_memory;       /* [mem_size]                                            */
    float *new_state_memory;    /* [mem_size, V (M/V+5)]                                 */
    uint8_t *terminal_memory;   /* [mem_size] 0/1                                        */
    int64_t mem_size, mem_cntr;
} RisVecSarlRollout;
int risvec_sarl_rollout(const RisVecState *s, const RisVecSarlParams *p, const RisVecSarlRollout *r,
                        const int32_t *arrivals, uint64_t seed, uint32_t counter, uint32_t flags,
                        risvec_stream_t stream);
/* 1 when the one-launch rollout step has a kernel for this shape, else 0 */
int risvec_sarl_rollout_supported(int32_t n_veh, int32_t n_ris);
/* sample_buffer (buffer.py:23-34) of the SARL ring whose pointers and mem_size `ring` holds (its other fields are not
 * read): rows idx[b] (int64, each < max_mem = min(mem_cntr, mem_size)) or, with idx NULL, the Philox draw of
 * risvec_replay_sample; state rows of state_dims floats, action rows of n_actions; outputs [batch, ...]. */
int risvec_sarl_replay_sample(const RisVecSarlRollout *ring, int32_t state_dims, int32_t n_actions, int64_t max_mem,
                              int32_t batch, const int64_t *idx, uint64_t seed, uint32_t counter, float *states,
                              float *actions, float *rewards, float *states_, uint8_t *dones, int64_t *idx_out,
                              risvec_stream_t stream);

/* BCD sweep + gains + step in one launch (BASELINE config 5: h_r read once into LDS). */
int risvec_step_fused_bcd(const RisVecState *s, const RisVecParams *p, const float *action,
                          const int32_t *partner, const int32_t *n_groups,
                          const int32_t *arrivals, uint64_t seed, uint32_t counter,
                          uint32_t flags, risvec_stream_t stream);

/* ===========================================================================================
 * NOMA grouping stage: the pairing the reference driver computes right before
 * every env.step() -- marl_train_bcd.py (TRAIN): feasibility mask TRAIN:128-156 + 842-855, score
 * matrix TRAIN:164-194, quantile-gated max-weight matching TRAIN:326-398, greedy completion
 * TRAIN:276-324, mask relaxation TRAIN:260-275, pair QoS check TRAIN:858-880, and the per-step
 * control logic with the freeze-in-episode safeties TRAIN:1401-1562, 1618-1623 -- for all E envs,
 * one wavefront per env, every comparison in float64 in the reference's association order.
 * n_veh <= 16.  Its outputs (partner / n_groups) are exactly what risvec_step* consume.
 * =========================================================================================== */
#define RISVEC_NOMA_MAX_VEH 16

typedef struct RisVecNomaParams {
    int32_t min_pair_target;        /* TRAIN:489   max(1, n_veh / 4); config.yaml 3        */
    int32_t mwm_backoff_rounds;     /* TRAIN:440 / 659                                      */
    int32_t mwm_allow_singles;      /* TRAIN:436                                            */
    int32_t qos_enable;             /* TRAIN:750   soft QoS penalty in the score            */
    int32_t relax_topk_step;        /* TRAIN:728                                            */
    int32_t freeze_group_in_episode;/* TRAIN:738                                            */
    int32_t freeze_recalc_every;    /* TRAIN:739   0 = frozen for the whole episode         */
    int32_t mask_enable;            /* TRAIN:498   0: pairing always sees the full mask     */
    double mwm_accept_quantile;     /* TRAIN:439                                            */
    double mwm_accept_q_step;       /* TRAIN:441                                            */
    double completion_min_quantile; /* TRAIN:282, 300                                       */
    double score_w_delta_db;        /* TRAIN:716                                            */
    double abs_gain_min_db;         /* TRAIN:723   (-inf = off)                             */
    double qos_soft_penalty;        /* TRAIN:172, 1450                                      */
    double qos_R_min;               /* TRAIN:751   bit/s/Hz                                 */
    double noise_power;             /* env.noise_power (ENV:72-76)                          */
    double P_max;                   /* env.P_max (ENV:125)                                  */
    double relax_tau_factor;        /* TRAIN:729                                            */
    double tau_back_floor_db;       /* TRAIN:1499                                           */
    double freeze_reward_drop_ratio;/* TRAIN:741                                            */
    double freeze_unstick_prob;     /* TRAIN:740                                            */
    float score_w_history;          /* TRAIN:717   (float32 product with the float32 history) */
    float pair_hist_decay;          /* TRAIN:719   (float32 in-place decay)                 */
} RisVecNomaParams;

enum RisVecNomaFlag {               /* bits of RisVecNomaState.flags[e]                     */
    RISVEC_NOMA_HAS_LAST = 1,       /* last_env_global is set (TRAIN:1298, 1618)            */
    RISVEC_NOMA_UNSTICK_USED = 2,   /* unstick_used_flag (TRAIN:1300, 1536)                 */
    RISVEC_NOMA_HAS_GROUPS = 4      /* episode_groups is set (TRAIN:1297, 1552)             */
};

/* Episode-scoped state of TRAIN:1282-1300, device pointers, N = n_veh.  Most steps of an episode
 * are frozen steps (TRAIN:1542-1547): for those risvec_noma_group only counts the step in `pending`;
 * the history decay / pair increments (TRAIN:1406, 1556-1558) and streak updates (TRAIN:1560-1561)
 * they owe are replayed, operation for operation, when the env next re-solves its pairing or when
 * risvec_noma_flush is called.  hist / streak are therefore current only after a flush; partner /
 * n_groups / flags always are. */
typedef struct RisVecNomaState {
    int32_t n_envs, n_veh;
    int64_t env_offset;             /* global id of local env 0 (RNG key)                   */
    float *hist;                    /* [E,N,N] pair_affinity_hist                           */
    int32_t *streak;                /* [E,N]   unpaired_streak                              */
    int32_t *partner;               /* [E,N]   episode_groups = this step's noma_groups, partner encoding of risvec_step */
    int32_t *n_groups;              /* [E]     len(episode_groups)                          */
    double *last_global;            /* [E]     last_env_global                              */
    double *best_global;            /* [E]     ep_env_best                                  */
    uint8_t *flags;                 /* [E]     RisVecNomaFlag bits                          */
    uint8_t *mask;                  /* [E,N,N] last_mask_mat (0/1)                          */
    double *tau;                    /* [E]     last_tau_now                                 */
    int32_t *pending;               /* [E]     frozen steps not yet applied to hist / streak */
    void *scratch;                  /* risvec_noma_scratch_bytes(E, N) bytes of ZEROED device memory (NULL when that is 0):
                                       beyond 8 vehicles risvec_noma_group is two launches, and this is the list of envs
                                       the first leaves to the second (a pairing graph too dense for its on-chip table) */
    int64_t scratch_bytes;
} RisVecNomaState;

/* Scratch risvec_noma_group needs for this batch: 0 up to 8 vehicles, 16 B + 4 B per env (rounded up to 256 B) beyond.
 * Zero it once when it is allocated (risvec_noma_begin_episode also empties the list); every call leaves it empty. */
int64_t risvec_noma_scratch_bytes(int32_t n_envs, int32_t n_veh);

void risvec_noma_default_params(RisVecNomaParams *p, int32_t n_veh);   /* driver Config defaults */

/* Start of an episode (TRAIN:1282-1300): zero hist / streak / flags / pending. */
int risvec_noma_begin_episode(const RisVecNomaState *ns, risvec_stream_t stream);

/* Channel-refresh step (TRAIN:1319-1343): tau = quantile q_now of |g_strong - g_weak| in dB
 * (TRAIN:842-855) -> ns->tau; with K_now >= 1 also the N x N mask (TRAIN:134-156) -> ns->mask.
 * gain [E,N] float32 linear; gdb15 [E,N] float64 = 10 log10(max(g, 1e-15)) or NULL (computed on
 * the device; pass it to reproduce a host's log10 bit for bit -- see EXPERIMENTS.md, section 8 f2). */
int risvec_noma_mask(const RisVecNomaState *ns, const float *gain, const double *gdb15, double q_now,
                     int32_t K_now, risvec_stream_t stream);

/* One pass of TRAIN:1401-1562 for every env; this step's noma_groups are left in ns->partner /
 * ns->n_groups, ready for risvec_step*.
 *   gain [E,N] f32; gdb12 [E,N] f64 = 10 log10(max(g, 1e-12)) or NULL; p_off01 [E,N] f32 = the
 *   offload power in [0,1] used by the QoS check (TRAIN:1391-1396; may be NULL when qos is off);
 *   use_mask: this step's mask_mat is ns->mask (a refresh step) / 0 = None (TRAIN:1421-1424);
 *   K_back, tau_back [E]: last_K_now / last_tau_now (TRAIN:1486-1491; last_q_now only feeds a
 *   value the reference computes and never uses, TRAIN:1497);
 *   prev_global (stride in floats) or NULL: global reward of the PREVIOUS step -- the
 *   ep_env_best / last_env_global bookkeeping of TRAIN:1618-1623 is applied first;
 *   u_unstick [E] f32 or NULL (Philox) : the draw of TRAIN:1539;
 *   info_out [E,4] or NULL: {recomputed, back-off rounds, pairs, matchable users of the last matching}. */
int risvec_noma_group(const RisVecNomaState *ns, const RisVecNomaParams *np, const float *gain,
                      const double *gdb12, const float *p_off01, int32_t use_mask, int32_t K_back,
                      const double *tau_back, const float *prev_global, int32_t prev_global_stride,
                      int32_t i_step, const float *u_unstick, uint64_t seed, uint32_t counter,
                      int32_t *info_out, risvec_stream_t stream);

/* risvec_noma_group reading the pairing power straight from the SAC power head: power_raw [E,N,2] in [-1,1], of which
 * component 0 is mapped as risvec_marshal_actions maps it (TRAIN:1391-1396, bit for bit) -- no marshalling launch. */
int risvec_noma_group_raw(const RisVecNomaState *ns, const RisVecNomaParams *np, const float *gain,
                          const double *gdb12, const float *power_raw, int32_t use_mask, int32_t K_back,
                          const double *tau_back, const float *prev_global, int32_t prev_global_stride,
                          int32_t i_step, const float *u_unstick, uint64_t seed, uint32_t counter,
                          int32_t *info_out, risvec_stream_t stream);

/* Apply the deferred frozen steps to hist / streak (pair_hist_decay = np->pair_hist_decay). */
int risvec_noma_flush(const RisVecNomaState *ns, const RisVecNomaParams *np, risvec_stream_t stream);

/* ===========================================================================================
 * Replay ring buffer + policy-output marshalling: buffer.py (BUF) kept in HBM and
 * fed straight from the step kernel's outputs, and the marshalling the driver does around
 * env.step() (TRAIN:1386-1396, 1601-1608, 1776-1799).
 * =========================================================================================== */
typedef struct RisVecReplay {            /* BUF:4-14; device pointers, row r of every array = transition r */
    int32_t n_agents, input_shape, n_actions;   /* state row = input_shape*n_agents floats, action row = n_actions*n_agents */
    int32_t reserved;
    int64_t mem_size;
    float *state_memory;                /* [mem_size, input_shape*n_agents]  */
    float *action_memory;               /* [mem_size, n_actions*n_agents]    */
    float *reward_global_memory;        /* [mem_size]                        */
    float *reward_local_memory;         /* [mem_size, n_agents]              */
    float *new_state_memory;            /* [mem_size, input_shape*n_agents]  */
    uint8_t *terminal_memory;           /* [mem_size] 0/1                    */
    float *mask_memory;                 /* [mem_size, n_agents*n_agents]     */
} RisVecReplay;

/* n consecutive store_transition calls (BUF:16-25), transition e landing in row (mem_cntr + e) % mem_size;
 * the caller advances its mem_cntr by n.  n <= mem_size.  reward_g is read with a stride (in floats) so
 * metrics[:,0] can be passed as is; done [n] 0/1 or NULL (then done_all applies to every transition);
 * mask [n, A*A] 0/1 bytes (the NOMA mask) or NULL = all ones (TRAIN:1786-1787); state_carry (or NULL)
 * receives a copy of state_ -- the next step's `state` (marl_state_old_all, TRAIN:1277) without a
 * separate copy; it must not alias state / state_. */
int risvec_replay_store(const RisVecReplay *rb, int64_t mem_cntr, int32_t n, const float *state, const float *action,
                        const float *reward_g, int32_t reward_g_stride, const float *reward_l, const float *state_,
                        const uint8_t *done, int32_t done_all, const uint8_t *mask, float *state_carry,
                        risvec_stream_t stream);

/* The rollout's transition store FUSED into the step (round 3): one launch runs step() (fused != 0: with the RIS
 * cascaded gains, as risvec_step_fused; 0: on the cached gains, as risvec_step) and appends this step's n_envs
 * transitions to the ring -- what risvec_step* followed by risvec_replay_store_policy do in two launches, bit for bit
 * (marl_train_bcd.py:1776-1799, buffer.py:16-25):
 *   state      <- state.obs as the kernel finds it (the observation the policy acted on: keep it current),
 *   action     <- per agent [probs_i with zero diagonal | raw power_i] from `action` (the raw policy output [E,V,2]:
 *                 flags must hold RISVEC_STEP_POLICY_ACTION | RISVEC_STEP_OBS) and ring->probs [E,V,V],
 *   reward_l / reward_g / state_ <- this step's per-user rewards, their mean, the new observation,
 *   done       <- ring->done for every transition, mask <- ring->mask [E,V,V] bytes or all ones when NULL.
 * Needs n_veh in {4, 8, 16}, rb.n_agents = n_veh, rb.input_shape = 5, rb.n_actions = n_veh + 2, n_envs <= mem_size;
 * fused != 0 additionally needs a shape with a software-pipelined kernel (RISVEC_ERR_UNSUPPORTED otherwise: use
 * the two-launch form).  The caller advances its mem_cntr by n_envs. */
typedef struct RisVecStepRing {
    RisVecReplay rb;
    int64_t mem_cntr;
    const float *probs;
    const uint8_t *mask;
    int32_t done;
    int32_t reserved;
} RisVecStepRing;
int risvec_step_ring(const RisVecState *s, const RisVecParams *p, const RisVecStepRing *ring, const float *action,
                     const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals, uint64_t seed,
                     uint32_t counter, uint32_t flags, int32_t fused, risvec_stream_t stream);

/* The fused step under a 3GPP channel model (phy.channel_model 3gpp_umi / 3gpp_uma / other; ENV:8-25, 255-327): ONE
 * launch does risvec_gain_3gpp(model, draws, seed, chan_counter) and then the step, bit for bit on every state tensor
 * and output:
 *   ring == NULL   risvec_gain_3gpp + risvec_step(..., counter, flags)
 *   ring != NULL   risvec_gain_3gpp + risvec_step_ring(..., fused = 0): the transition store too (needs n_veh in
 *                  {4, 8, 16} and flags with RISVEC_STEP_POLICY_ACTION | RISVEC_STEP_OBS, as risvec_step_ring)
 * The gains are computed in registers from state.pos and also written to state.gain.  h_r, theta, b and pl are not
 * read, so any n_veh <= 64 and any n_ris is served.  model: RISVEC_CH_3GPP_UMI, _UMA or _OTHER (0 dB path loss);
 * RISVEC_CH_FREE is rejected (the RIS entry points serve it).  fading: injected draws or NULL (Philox, Rayleigh or
 * Rice per p->rician_k_db, as risvec_gain_3gpp).  flags: RISVEC_STEP_METRICS / _POWER_W / _OBS / _POLICY_ACTION only.
 * risvec_step_kernel(s, flags | RISVEC_STEP_3GPP, RISVEC_FORM_FUSED / _FUSED_RING / _FUSED_MULTI) names the kernel. */
typedef struct RisVecFading {
    const float *u_los;     /* u_los ~ U[0,1), z_shadow ~ N(0,1), small = small-scale power; [E,V] float32 each  */
    const float *z_shadow;  /* ([T,E,V] for risvec_step_fused_3gpp_multi); all three or none (NULL: Philox)      */
    const float *small;
} RisVecFading;
int risvec_step_fused_3gpp(const RisVecState *s, const RisVecParams *p, int32_t model, const float *action,
                           const int32_t *partner, const int32_t *n_groups, const int32_t *arrivals,
                           const RisVecFading *fading, uint64_t seed, uint32_t counter, uint32_t chan_counter,
                           uint32_t flags, const RisVecStepRing *ring, risvec_stream_t stream);

/* n_steps risvec_step_fused_3gpp calls (ring = NULL) in ONE launch: step t draws its fading with chan_counter + t and
 * its arrivals with counter + t (or reads slice t of the injected [T,E,V] draws and arrivals), i.e. the counters T
 * single calls would use.  Positions cannot change inside the launch, so distances, LOS probability and both path
 * losses are computed once; the LOS decision, shadow and small-scale power are drawn every step.  Records and final
 * state as risvec_step_fused_multi; state.gain ends up holding the last step's gains. */
int risvec_step_fused_3gpp_multi(const RisVecState *s, const RisVecParams *p, int32_t model, int32_t n_steps,
                                 const float *actions, const int32_t *partner, const int32_t *n_groups,
                                 const int32_t *arrivals, const RisVecFading *fading, uint64_t seed, uint32_t counter,
                                 uint32_t chan_counter, const RisVecTraj *traj, uint32_t flags, risvec_stream_t stream);


/* risvec_replay_store with the action row built in the store kernel from the policy outputs -- power_raw [n,A,2],
 * probs [n,A,A]: per agent [probs_i with zero diagonal | raw power_i], exactly the action_store row of
 * risvec_marshal_actions (TRAIN:1386-1390, 1776-1784) -- so a rollout step needs no marshalling launch: the env
 * takes power_raw with RISVEC_STEP_POLICY_ACTION, the grouping takes it through risvec_noma_group_raw.
 * Needs n_actions = n_agents + 2. */
int risvec_replay_store_policy(const RisVecReplay *rb, int64_t mem_cntr, int32_t n, const float *state,
                               const float *power_raw, const float *probs, const float *reward_g,
                               int32_t reward_g_stride, const float *reward_l, const float *state_, const uint8_t *done,
                               int32_t done_all, const uint8_t *mask, float *state_carry, risvec_stream_t stream);

/* sample_buffer (BUF:27-37): rows idx[b] (int64, each < max_mem = min(mem_cntr, mem_size)) or, with
 * idx NULL, Philox(seed; b, 0, counter, site 8) -> floor(x * max_mem / 2^32); outputs [batch, ...] in the
 * order sample_buffer returns them; idx_out (or NULL) receives the rows used. */
int risvec_replay_sample(const RisVecReplay *rb, int64_t max_mem, int32_t batch, const int64_t *idx, uint64_t seed,
                         uint32_t counter, float *states, float *actions, float *rewards_g, float *rewards_l,
                         float *states_, uint8_t *dones, float *masks, int64_t *idx_out, risvec_stream_t stream);

/* Policy outputs -> the three places the driver sends them: power_raw [E,V,2] (SAC power head, in
 * [-1,1]), probs [E,V,V] (intent probabilities) ->
 *   action_env   [E,2,V]      TRAIN:1601-1608  clip to +-0.999, (x+1)/2, CPU share floored at clamp(floor,0,0.95)
 *   p_off01      [E,V]        TRAIN:1391-1396  (input of the NOMA QoS check)
 *   action_store [E,V*(V+2)]  TRAIN:1386-1390, 1776-1784  per agent [probs_i with zero diagonal, raw power_i]
 * any output may be NULL; probs may be NULL when action_store is. */
int risvec_marshal_actions(int32_t n_envs, int32_t n_veh, const float *power_raw, const float *probs,
                           float cpu_share_floor, float *action_env, float *p_off01, float *action_store,
                           risvec_stream_t stream);

/* Batched choose_action, sampling epilogue (sac_agent.py:80-131, 187-225) + marshalling in one
 * launch.  heads [V, E, 4+V] float32 = per agent the rows (mu[2], log_std[2], intent_logits[V]) its
 * PolicyNetwork.forward produced (sac_agent.py:62-78: three small GEMMs, library work); mask [E,V,V] 0/1
 * bytes or NULL; tau [V] the agents' Gumbel temperatures; hard [V] bytes or NULL: per agent the straight-through
 * one-hot form of F.gumbel_softmax (marl_train_bcd.py:1816-1818); eps [E,V,2] ~ N(0,1) and expo [E,V,V] ~ Exp(1)
 * inject the draws of Normal.sample / F.gumbel_softmax (NULL: Philox keyed by env_offset + e).
 * Outputs: power_raw [E,V,2] (tanh-squashed), probs [E,V,V] (soft Gumbel-softmax), onehot [E,V,V] or
 * NULL; and, each optional, exactly what risvec_marshal_actions would produce from them:
 * action_env [E,2,V], p_off01 [E,V], action_store [E,V*(V+2)]. */
int risvec_policy_sample(int32_t n_envs, int32_t n_veh, int64_t env_offset, const float *heads, const uint8_t *mask,
                         const float *tau, const uint8_t *hard, const float *eps, const float *expo, uint64_t seed,
                         uint32_t counter, float cpu_share_floor, float *power_raw, float *probs, float *onehot,
                         float *action_env, float *p_off01, float *action_store, risvec_stream_t stream);

/* The learner's policy.sample_normal(obs_j, mask=mask_j) (sac_agent.py:80-127) for every sampled row and agent, with
 * what global_learn does with it (global_sac_critic.py:326-336), in one launch.  heads [V, B, 4+V], mask [B,V,V] or
 * NULL, tau [V], hard [V] or NULL, eps [B,V,2] / expo [B,V,V] (NULL: Philox keyed by row_offset + b, the sites, block
 * -> value mapping and 2^-24 floor of risvec_policy_sample) as for risvec_policy_sample, and for the same heads and
 * draws power / probs / the arg-max are that entry point's power_raw / probs / onehot bit for bit.
 * Outputs, each optional (NULL: not written; at least one must be given):
 *   power [B,V,2], probs [B,V,V] (y, soft or straight-through per hard[v]),
 *   next_actions [B, V*(V+2)]  per agent [onehot(argmax y) (V), power (2)]: the target critics' action input,
 *   logp_power [B,V]   = sum_i ( -eps_i^2/2 - log_std_i - log(2 pi)/2 - log(1 - p_i^2 + 1e-6) ), from the draw eps
 *                        itself (equal to the reference's (x_t - mu)^2 / (2 var) form without its cancellation),
 *   logp_intent [B,V]  = sum_k y_k lsm_k, or lsm[argmax y] where hard[v]; lsm = log_softmax(masked logits),
 *   logp_power_sum [B], logp_intent_sum [B]: the float32 sums over the agents in agent order 0..V-1 (no atomics);
 *                        n_veh <= 16 only -- with more agents a non-NULL sum pointer is RISVEC_ERR_ARG.
 * n_rows == 0 returns RISVEC_OK without a launch; every other invalid argument is RISVEC_ERR_ARG. */
int risvec_policy_sample_normal(int32_t n_rows, int32_t n_veh, int64_t row_offset, const float *heads, const uint8_t *mask,
                                const float *tau, const uint8_t *hard, const float *eps, const float *expo, uint64_t seed,
                                uint32_t counter, float *power, float *probs, float *next_actions, float *logp_power,
                                float *logp_intent, float *logp_power_sum, float *logp_intent_sum, risvec_stream_t stream);

/* The two non-GEMM ends of PolicyNetwork.forward (sac_agent.py:62-78), all agents and envs per launch;
 * the fc1 x fc2 product in between is a plain batched GEMM (rocBLAS).  Row-major float32 everywhere.
 *   layer1: obs [E,V,in] , W1 [V,in,F1] (= fc1.weight^T), b1 / ln_w / ln_b [V,F1]
 *           -> out [V,E,F1] = relu(LayerNorm(fc1(obs)))                      (F1 <= 1024; in*F1 must fit LDS)
 *   heads : g [V,E,F2] (= fc2 product; b2 [V,F2] its bias, added here, or NULL), ln_w / ln_b [V,F2], Wh [V,F2,H] (= [mu|log_std|intent_logits]
 *           weights transposed, H = 4 + V), bh [V,H]
 *           -> heads [V,E,H], the input of risvec_policy_sample                (F2 <= 1024) */
int risvec_policy_layer1(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, const float *obs, const float *W1,
                         const float *b1, const float *ln_w, const float *ln_b, float *out, risvec_stream_t stream);
/* risvec_policy_layer1 writing the hidden row as the float16 operand of a split-precision GEMM: out16
 * [V, E, 3*f1] halfs, row = [ hi(h) | hi(h) 2^-5 | (h - hi(h)) 2^6 ] with hi = round-to-nearest float16.
 * Multiplied (float16 inputs, float32 accumulation) by the fc2 weight stacked along K as
 * [ hi(W) ; (W - hi(W)) 2^5 ; hi(W) 2^-6 ] it gives h W to 2^-22 relative per product -- the accuracy of the
 * float32 GEMM at the fp16 matrix-core rate.  f1 must be a multiple of 4, in_dims <= 8.  |h| must stay below
 * the float16 maximum 65504 (LayerNorm outputs do). */
int risvec_policy_layer1_split16(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, const float *obs,
                                 const float *W1, const float *b1, const float *ln_w, const float *ln_b, void *out16,
                                 risvec_stream_t stream);
/* The whole PolicyNetwork.forward (sac_agent.py:62-78) of every agent in ONE launch, all three layers on the
 * fp16 matrix cores at float32 accuracy (every operand split into float16 hi + lo, the three significant partial
 * products accumulated in float32); neither hidden layer touches HBM.  Prepared weights (rebuild after an update),
 * "fragment" = the 8 halfs one lane feeds to v_mfma_f32_32x32x16_f16, S_0 = hi(2^s X), S_1 = fp16(2^s X - S_0), s a
 * per-agent power of two that keeps S_1 in the float16 normal range:
 *   G    [V, 6, 6]  C C^T / f1, C = fc1 weight rows (and the bias as row in_dims) centred over the feature axis:
 *                   LayerNorm-1 variance of an env in closed form, var = x^T G x with x = (obs, 1, 0..);
 *   fc1 operand     X = [f1, 16]: column k < in_dims = C[k] ln1_w, column in_dims = C[in_dims] ln1_w, column in_dims + 1
 *                   = ln1_b, rest 0 (multiplied by (obs rstd, rstd, 1, 0..) it gives the normalised pre-activation);
 *                   fragments of group g (32 features): element (t, lane, j) = S_t[32g + (lane&31)][8(lane>>5) + j];
 *   W1F  [V, 2, 64, 8]  the fc1-operand fragments of group 0;
 *   W2f  [V, f1/32, 8 + 4 f2/32, 64, 8]  the weight stream, per group g of 32 hidden features: 8 fragment rows holding
 *                   the fc1-operand fragments of group g+1 (rows 0-1; rest padding), then for k-steps u = 0, 1 the
 *                   fc2 weight X = W2 [f1, f2] in the k order in which the fc2 MFMA reads the fc1 MFMA's accumulator:
 *                   rows [t][m], element (lane, j) = S_t[32g + 16u + 8(j>>2) + 4(lane>>5) + (j&3)][32m + (lane&31)];
 *   w_unscale [V]   2^-(s_fc1 + s_fc2);
 *   WhF  [V, f2/32, 2, 2, 64, 8]  X = the head weight Wh [f2, n_heads] (columns mu | log_std | intent_logits) zero-padded
 *                   to 32 columns: element (m, u, t, lane, j) = S_t[32m + 16u + 8(j>>2) + 4(lane>>5) + (j&3)][lane&31];
 *   wh_unscale [V]  its 2^-s.
 * heads [V, E, n_heads].  Built for in_dims <= 5, f1 % 32 == 0 <= 1024, f2 in {128, 256}, n_heads <= 24
 * (risvec_policy_mlp_supported); other shapes return RISVEC_ERR_UNSUPPORTED -- use the three-launch form. */
int risvec_policy_mlp_supported(int32_t in_dims, int32_t f1, int32_t f2, int32_t n_heads);
int risvec_policy_mlp(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, int32_t f2, int32_t n_heads, const float *obs,
                      const float *G, const void *W1F, const void *W2f, const float *w_unscale, const float *b2,
                      const float *ln2_w, const float *ln2_b, const void *WhF, const float *wh_unscale, const float *bh,
                      float *heads, risvec_stream_t stream);
/* The single-agent (DDPG) actor, ActorNetwork.forward (Simulation-SARL/networks.py:132-141): x [n_rows, in_dims] ->
 * fc1 -> LayerNorm -> ReLU -> fc2 -> LayerNorm -> ReLU -> mu -> sigmoid, in ONE launch with one weight set shared by all
 * rows, every product on the fp16 matrix cores at float32 accuracy (operands split as for risvec_policy_mlp); neither
 * hidden layer touches memory.  mu [n_rows, n_actions] = sigmoid(logits); logits [n_rows, n_actions] (optional) receives
 * the pre-sigmoid values.  x viewed as [E, V (M/V + 5)] is the observation the rollout launch writes, and mu is the
 * tensor it reads, both in place.  16-byte alignment of x rows is needed only through the base pointer.
 * Prepared weights (rebuild after an update; S_0 / S_1 = float16 hi / lo of 2^s X, s one power of two per matrix):
 *   wstream  `items` items of `rows` fragment rows [64 lanes][8 halfs] (1 KiB), with KS = the first of {3, 6, 7, 9} >=
 *            ceil((in_dims + 1) / 16), MT = fc2 / 32, HT = ceil(n_actions / 32), NG = fc1 / 32,
 *            rows = 2 KS + 1 + 4 MT rounded up to a multiple of 4, P1 = rows / (2 KS), HS = rows / (2 HT):
 *     ceil(NG / P1) pass-1 items: group g (32 fc1 features) in item g / P1 at rows 2 KS (g % P1) + 2 s + t, element
 *            (lane, j) = S_t[32 g + (lane & 31)][16 s + 8 (lane >> 5) + j] of X = the fc1 weight [fc1, 16 KS] with the bias as
 *            column in_dims, centred over the feature axis (every column sums to zero over fc1), zero beyond;
 *     NG pass-2 items: rows [0, 2 KS) group g's fc1 fragments again; row 2 KS = LayerNorm-1 weight [32] and bias [32] of the
 *            group as float32; rows 2 KS + 1 + (2 u + t) MT + m, element (lane, j) =
 *            S_t[32 g + 16 u + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)][32 m + (lane & 31)] of X = the fc2 weight [fc1, fc2];
 *     ceil(2 MT / HS) head items: k-step st = 2 m + u in item st / HS at rows 2 HT (st % HS) + 2 ht + t, element (lane, j) =
 *            S_t[32 m + 16 u + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)][32 ht + (lane & 31)] of X = the mu weight [fc2, 32 HT]
 *            (zero padded); unused rows are zero;
 *   wstream_bytes  its size, checked against the shape;
 *   scales [3]  2^-s of fc1, fc2 and mu.
 * Built for in_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256}, n_actions <= 96 (risvec_sarl_actor_supported, host
 * only); other shapes return RISVEC_ERR_SHAPE.  Inputs beyond the float16 range (|x| > 65504) are not supported. */
int risvec_sarl_actor_supported(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions);
int risvec_sarl_actor(int32_t n_rows, int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions, const float *x,
                      const void *wstream, int64_t wstream_bytes, const float *scales, const float *b2, const float *ln2_w,
                      const float *ln2_b, const float *bmu, float *logits, float *mu, risvec_stream_t stream);
/* The prepared weights of risvec_sarl_actor, built on the device from the float32 weights as the learner holds them
 * (Linear weights [out, in]: W1 [fc1, in_dims], b1 [fc1], W2 [fc2, fc1], Wmu [n_actions, fc2]; LayerNorm-1 ln1_w, ln1_b
 * [fc1]), read in place: call it after every optimiser step.  Two launches on `stream`, no allocation, no
 * synchronisation: one workgroup takes the float64 mean over the features of every row of [W1^T ; b1], the largest
 * magnitude of the centred fc1 operand, of W2 and of Wmu, and from them s = floor(log2(64 / max(amax, 1e-30))) clamped to
 * [-40, 40] per matrix; the second launch writes every 16-byte fragment of the layout above exactly once, padding
 * included (the buffer may hold anything before the call): centre in float64, scale by 2^s, round to float32,
 * S_0 = half(x), S_1 = half(x - float(S_0)).  Sums run in a fixed order: the same bits on every call.
 *   wstream, wstream_bytes  the stream to write and its size, checked against the shape;
 *   scales [3]              receives 2^-s of fc1, fc2 and mu;
 *   workspace               risvec_sarl_actor_pack_workspace bytes (0: a shape risvec_sarl_actor is not built for), of
 *                           any content; holds the means and 2^s between the launches.
 * Shapes outside risvec_sarl_actor_supported return RISVEC_ERR_UNSUPPORTED. */
size_t risvec_sarl_actor_pack_workspace(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions);
int risvec_sarl_actor_pack(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions, const float *W1, const float *b1,
                           const float *ln1_w, const float *ln1_b, const float *W2, const float *Wmu, void *wstream,
                           size_t wstream_bytes, float *scales, void *workspace, size_t workspace_bytes,
                           risvec_stream_t stream);
/* The single-agent (DDPG) critic, CriticNetwork.forward (Simulation-SARL/networks.py:66-79), and the TD target of learn()
 * (ddpg_torch.py:84-88), in ONE launch with one weight set shared by all rows:
 *     s = relu(LN1(fc1 x));  s = LN2(fc2 s);  h = relu(s + action_value(a));  h = relu(LN3(fc3 h));  q = q_w . h + q_b
 *     y[row] = done[row] ? reward[row] : reward[row] + gamma q[row]      (a select; one fused multiply-add)
 * x [n_rows, in_dims], a [n_rows, n_actions] float32, read in place (no alignment beyond float's).  The four matrix products
 * run on the fp16 matrix cores at float32 accuracy (operands split as for risvec_sarl_actor), the 1-wide q layer is a dot
 * product in registers; no hidden layer touches memory.  q_out [n_rows] and y_out [n_rows] are each optional, at least one
 * must be given; y_out needs reward [n_rows] float32 and done [n_rows] uint8 (0 / 1).
 * Prepared weights (rebuild after an update; S_0 / S_1 = float16 hi / lo of 2^s X, s one power of two per matrix):
 *   wstream  fragment rows [64 lanes][8 halfs] (1 KiB) in four blocks, with KS = ceil((in_dims + 1) / 16), KSA =
 *            ceil(n_actions / 16), NG = fc1 / 32, MT2 = fc2 / 128, MT3 = fc3 / 128; w < 4 is the wavefront that owns
 *            output tiles [w MT, (w + 1) MT) of a layer, t = hi / lo:
 *     action_value  row ((w KSA + s) MT2 + m) 2 + t: element (lane, j) = S_t[16 s + 8 (lane >> 5) + j][32 (w MT2 + m) + (lane & 31)]
 *            of X = the action_value weight as [16 KSA, fc2], zero beyond n_actions;
 *     fc1    row (g KS + s) 2 + t, g < NG: element (lane, j) = S_t[32 g + (lane & 31)][16 s + 8 (lane >> 5) + j] of X = the fc1
 *            weight [fc1, 16 KS] with the bias as column in_dims, centred over the feature axis (every column sums to
 *            zero over fc1), zero beyond;
 *     fc2    row ((w 2 NG + k) MT2 + m) 2 + t, k < 2 NG: element (lane, j) =
 *            S_t[16 k + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)][32 (w MT2 + m) + (lane & 31)] of X = the fc2 weight [fc1, fc2];
 *     fc3    row ((w fc2 / 16 + k) MT3 + m) 2 + t, k < fc2 / 16: the same element rule for X = the fc3 weight [fc2, fc3];
 *   wstream_bytes  its size = risvec_sarl_critic_stream_bytes(...), checked against the shape;
 *   scales [4]  2^-s of fc1, fc2, action_value and fc3;
 *   ln1_w, ln1_b [fc1]; b2, ln2_w, ln2_b, bav (the action_value bias) [fc2]; b3, ln3_w, ln3_b, q_w [fc3]; q_b [1]: float32,
 *            16-byte aligned, read in place.
 * Built for in_dims <= 128, fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}, n_actions <= 96
 * (risvec_sarl_critic_supported, host only); other shapes return RISVEC_ERR_SHAPE (stream_bytes: 0).  Inputs beyond the
 * float16 range (|x| > 65504) are not supported. */
int risvec_sarl_critic_supported(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions);
int64_t risvec_sarl_critic_stream_bytes(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions);
int risvec_sarl_critic(int32_t n_rows, int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions, const float *x,
                       const float *a, const void *wstream, int64_t wstream_bytes, const float *scales, const float *ln1_w,
                       const float *ln1_b, const float *b2, const float *ln2_w, const float *ln2_b, const float *bav,
                       const float *b3, const float *ln3_w, const float *ln3_b, const float *q_w, const float *q_b,
                       const float *reward, const uint8_t *done, float gamma, float *q_out, float *y_out,
                       risvec_stream_t stream);
/* The prepared weights of risvec_sarl_critic, built on the device from the float32 weights as the learner holds them
 * (Linear weights [out, in]: W1 [fc1, in_dims], b1 [fc1], W2 [fc2, fc1], Wav [fc2, n_actions], W3 [fc3, fc2]), read in
 * place: call it after every update of the target critic.  Two launches on `stream`, no allocation, no synchronisation.
 * The first takes, in one workgroup, the float64 mean over the features of every row of [W1^T ; b1] and the largest
 * magnitude of the centred fc1 operand, and in further workgroups the largest magnitudes of slices of W2, Wav and W3,
 * one workspace slot per slice (no atomics, nothing to initialise).  The second combines the slots into
 * s = floor(log2(64 / max(amax, 1e-30))) clamped to [-40, 40] per matrix (quotient and logarithm in float64 for fc1, in
 * float32 for the others) and writes every 16-byte fragment of the layout above exactly once, padding included (the
 * buffer may hold anything before the call): centre in float64 (fc1), scale by 2^s, round to float32, S_0 = half(x),
 * S_1 = half(x - float(S_0)).  Sums run in a fixed order: the same bits on every call.
 *   W1, b1, W2, Wav, W3     float-aligned (16-byte alignment of W2 and W3 lets their fragments be read as float4);
 *   wstream, wstream_bytes  the stream to write, 16-byte aligned, and its size = risvec_sarl_critic_stream_bytes(...);
 *   scales [4]              receives 2^-s of fc1, fc2, action_value and fc3;
 *   workspace               risvec_sarl_critic_pack_workspace bytes (0: a shape risvec_sarl_critic is not built for),
 *                           16-byte aligned, of any content; holds the means and the maxima between the launches.
 * Shapes outside risvec_sarl_critic_supported return RISVEC_ERR_UNSUPPORTED. */
size_t risvec_sarl_critic_pack_workspace(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions);
int risvec_sarl_critic_pack(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions, const float *W1,
                            const float *b1, const float *W2, const float *Wav, const float *W3, void *wstream,
                            size_t wstream_bytes, float *scales, void *workspace, size_t workspace_bytes,
                            risvec_stream_t stream);
/* The multi-agent (SAC) twin global critic and the TD target of Global_SAC_Critic.global_learn
 * (Simulation-MARL-BCD/global_sac_critic.py:338-352; the network: networks.py:7-49, a plain ReLU MLP on cat([state, action])),
 * in ONE launch for n_rows rows and n_nets in {1, 2} weight sets of one shape:
 *     x   = [state[row, 0:state_dims] | action[row, 0:action_dims]]        two pointers, read in place
 *     h1  = relu(W1 x + b1);  h2 = relu(W2 h1 + b2);  h3 = relu(W3 h2 + b3);  q_c = qw . h3 + qb          c = 1 .. n_nets
 *     m   = n_nets == 2 ? min(q_1, q_2) : q_1
 *     ent = coef[0] logp_power[row] + coef[1] logp_intent[row]             a term whose logp pointer is NULL is absent
 *     y[row] = done[row] ? reward[row] : reward[row] + gamma (m - ent)     (a select; the last step one fused multiply-add)
 * state [n_rows, state_dims], action [n_rows, action_dims], reward, logp_power, logp_intent [n_rows] float32, done
 * [n_rows] uint8 (0 / 1), coef [2] float32 ON THE DEVICE (the learner's log_alpha.exp() * entropy_scale: the single-alpha
 * path passes the same value twice), all read in place with no alignment beyond their type's.  q1, q2, y [n_rows] are
 * each optional (NULL: not written), at least one must be given; q2 needs n_nets == 2; y needs reward and done; a logp
 * pointer needs coef and y.  n_nets == 1 is the plain forward of one CriticNetwork (the local critics of sac_agent.py).
 * One launch on `stream`: no atomics, no second pass, no workspace, no synchronisation.  The three matrix products run on
 * the fp16 matrix cores at float32 accuracy (operands split as for risvec_sarl_critic), the 1-wide q layer is a dot
 * product in registers; no hidden layer and no concatenated input touches memory.
 * Prepared weights of one net (rebuild after an update; S_0 / S_1 = float16 hi / lo of 2^s X, s one power of two per matrix):
 *   wstream  fragment rows [64 lanes][8 halfs] (1 KiB) in three blocks, with KS = ceil((state_dims + action_dims) / 16),
 *            NG = fc1 / 32, MT2 = fc2 / 128, MT3 = fc3 / 128; w < 4 is the wavefront that owns output tiles
 *            [w MT, (w + 1) MT) of a layer, t = hi / lo:
 *     fc1    row (g KS + s) 2 + t, g < NG: element (lane, j) = S_t[32 g + (lane & 31)][16 s + 8 (lane >> 5) + j] of X = the fc1
 *            weight [fc1, 16 KS], zero beyond state_dims + action_dims;
 *     fc2    row ((w 2 NG + k) MT2 + m) 2 + t, k < 2 NG: element (lane, j) =
 *            S_t[16 k + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)][32 (w MT2 + m) + (lane & 31)] of X = the fc2 weight [fc1, fc2];
 *     fc3    row ((w fc2 / 16 + k) MT3 + m) 2 + t, k < fc2 / 16: the same element rule for X = the fc3 weight [fc2, fc3];
 *   wstream_bytes  its size = risvec_marl_critic_stream_bytes(...), checked against the shape;
 *   scales [3]  2^-s of fc1, fc2 and fc3;
 *   b1 [fc1], b2 [fc2], b3 [fc3], qw [fc3], qb [1]: float32, 16-byte aligned, read in place.
 * Built for state_dims + action_dims <= 128 (each >= 1), fc1 % 32 == 0 <= 1024, fc2 in {128, 256, 512}, fc3 in {128, 256}
 * (risvec_marl_critic_supported, host only); other shapes return RISVEC_ERR_UNSUPPORTED (stream_bytes: 0).  Every other
 * argument error returns RISVEC_ERR_ARG; all are reported before anything is launched and without touching a device.
 * Inputs beyond the float16 range (|x| > 65504) are not supported. */
typedef struct RisVecMarlCriticNet {
    const void *wstream;
    int64_t wstream_bytes;
    const float *scales;
    const float *b1, *b2, *b3, *qw, *qb;
} RisVecMarlCriticNet;
int risvec_marl_critic_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
int64_t risvec_marl_critic_stream_bytes(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
int risvec_marl_critic(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                       int32_t n_nets, const RisVecMarlCriticNet *nets, const float *state, const float *action,
                       const float *reward, const uint8_t *done, float gamma, const float *coef, const float *logp_power,
                       const float *logp_intent, float *q1, float *q2, float *y, risvec_stream_t stream);
/* The prepared weights of risvec_marl_critic for n_nets in {1, 2} nets of one shape, built on the device from the float32
 * weights as the learner holds them (Linear weights [out, in]), read in place: call it after every update of the target
 * critics (each call of update_global_network_parameters, global_sac_critic.py:394-400).  Two launches on `stream` for
 * all nets together, no allocation, no synchronisation.  The first takes the largest magnitudes of slices of W1, W2 and
 * W3 of every net, one workspace slot per net, matrix and slice (one writer per slot, every slot written: no atomics,
 * nothing to initialise).  The second combines the slots into s = floor(log2f(64 / max(amax, 1e-30))) clamped to
 * [-40, 40] per net and matrix -- quotient and logarithm in float32 for all three matrices -- and writes every 16-byte
 * fragment of the layout above exactly once, padding included (the buffers may hold anything before the call): scale
 * by 2^s in float64, round to float32, S_0 = half(x), S_1 = half(x - float(S_0)).  A maximum does not depend on the order
 * it is taken in and everything else is exact or correctly rounded: the same bits on every call.
 *   W1, W2, W3     [fc1, state_dims + action_dims], [fc2, fc1], [fc3, fc2]: float-aligned (W2 and W3 of every net on 16
 *                  bytes lets their fragments be read as float4);
 *   wstream, wstream_bytes  the stream to write, 16-byte aligned, and its size = risvec_marl_critic_stream_bytes(...);
 *   scales [3]     receives 2^-s of fc1, fc2 and fc3;
 *   workspace      risvec_marl_critic_pack_workspace bytes (0: a shape risvec_marl_critic is not built for, or n_nets
 *                  outside {1, 2}), 16-byte aligned, of any content; holds the maxima between the launches.
 * Shapes outside risvec_marl_critic_supported return RISVEC_ERR_UNSUPPORTED.  A NULL or misaligned pointer, n_nets
 * outside {1, 2}, a wrong wstream_bytes, too small a workspace and two nets that name the same wstream or the same
 * scales return RISVEC_ERR_ARG; all are reported before anything is launched and without touching a device. */
typedef struct RisVecMarlCriticPackNet {
    const float *W1, *W2, *W3;
    void *wstream;
    int64_t wstream_bytes;
    float *scales;
} RisVecMarlCriticPackNet;
size_t risvec_marl_critic_pack_workspace(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                                         int32_t n_nets);
int risvec_marl_critic_pack(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_nets,
                            const RisVecMarlCriticPackNet *nets, void *workspace, size_t workspace_bytes,
                            risvec_stream_t stream);
/* risvec_marl_critic for inputs that do not fit in LDS beside the activations: the same computation, arguments, weight
 * stream (the layout above at this shape's KS), outputs, checks and error codes, in ONE launch, with fc1 walking the input
 * in chunks of 8 k-steps (128 inputs) while a wavefront keeps the accumulators of all its fc1 groups in registers; every
 * net stages the input again, chunk by chunk.  Built for state_dims + action_dims <= 512 (each >= 1) and the fc rule of
 * risvec_marl_critic (risvec_marl_critic_wide_supported, host only) -- 16 vehicles are (80, 288) -- which deliberately
 * overlaps risvec_marl_critic_supported: within a group the k-steps are added in the same order into one accumulator, so
 * on a shape both cover the two entries give the same bits.  risvec_marl_critic_wide_stream_bytes is ONE net's stream
 * size under this rule (0: not built); risvec_marl_critic_wide_pack_workspace / risvec_marl_critic_wide_pack are
 * risvec_marl_critic_pack_workspace / risvec_marl_critic_pack -- the same two kernels, the same bits -- behind this
 * rule.  Nothing about risvec_marl_critic or its rule changes. */
int risvec_marl_critic_wide_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
int64_t risvec_marl_critic_wide_stream_bytes(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
int risvec_marl_critic_wide(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                            int32_t n_nets, const RisVecMarlCriticNet *nets, const float *state, const float *action,
                            const float *reward, const uint8_t *done, float gamma, const float *coef, const float *logp_power,
                            const float *logp_intent, float *q1, float *q2, float *y, risvec_stream_t stream);
size_t risvec_marl_critic_wide_pack_workspace(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                                              int32_t n_nets);
int risvec_marl_critic_wide_pack(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_nets,
                                 const RisVecMarlCriticPackNet *nets, void *workspace, size_t workspace_bytes,
                                 risvec_stream_t stream);
/* The critic loss of the multi-agent (SAC) learner and its gradients (Global_SAC_Critic.global_learn,
 * Simulation-MARL-BCD/global_sac_critic.py:355-363: q1, q2 = the online critics, loss = mse(q1, y) + mse(q2, y),
 * loss.backward()) without an autograd graph, in TWO launches on `stream` for n_rows rows and n_nets in {1, 2} nets of one
 * shape, per net c:
 *     e = (2 / n_rows) (q_c - target)                         target [n_rows]: a constant, read in place
 *     loss[0] = sum_c (1 / n_rows) sum_b (q_c[b] - target[b])^2
 *     d3 = (e qw) [h3 > 0]   d2 = (W3^T d3) [h2 > 0]   d1 = (W2^T d2) [h1 > 0]              (relu backward: out > 0)
 *     dqw = sum_b e h3   dqb = sum_b e   dWl = dl^T a(l-1) (a0 = [state | action])   dbl = sum_b dl
 * The gradients are OVERWRITTEN, never accumulated (zero_grad(set_to_none=True) and one backward()), every byte of them.
 * Launch 1 (grid: 32-row tiles x nets) walks the forward of risvec_marl_critic on the packed stream, leaves every
 * activation in the workspace, back-propagates the deltas within the workgroup -- the transposed products read the float32
 * W2 and W3 IN PLACE, scaled by the power of two that `scales` records and split on the fly -- and writes q1 / q2.  Launch
 * 2 runs one wavefront per 32 x 32 tile of every dWl over the batch; a few more wavefronts sum dqw, dqb and the loss in
 * float64.  Deltas are multiplied by an exact power of two (per tile in launch 1, per layer and net in launch 2) that
 * brings their largest entry into [64, 128) before the float16 split and the accumulator is multiplied back, so the
 * accuracy is the forward's at any size of the TD error.  No atomics: every output element has one writer that sums in a
 * fixed order, and every call gives the same bits.  No synchronisation, no allocation.
 *   nets[c].fwd    the net as risvec_marl_critic takes it: a stream that is current for W1, W2, W3;
 *   nets[c].W2 / W3  the float32 Linear weights [fc2, fc1] / [fc3, fc2] behind that stream, float-aligned;
 *   grads[c]       dW1 [fc1, state_dims + action_dims], db1 [fc1], dW2 [fc2, fc1], db2 [fc2], dW3 [fc3, fc2], db3 [fc3],
 *                  dqw [fc3], dqb [1]: float-aligned, all distinct;
 *   state, action  as for risvec_marl_critic; no row >= n_rows of state, action or target is read;
 *   q1, q2 [n_rows]  receive q_c; q2 with n_nets == 2 only (and then required);
 *   workspace      risvec_marl_critic_grad_workspace(n_rows, ...) bytes (0: n_rows < 1, a shape that is not built, or
 *                  n_nets outside {1, 2}), 16-byte aligned, of any content.
 * Built for the shapes of risvec_marl_critic (risvec_marl_critic_grad_supported, host only); other shapes return
 * RISVEC_ERR_UNSUPPORTED.  A NULL or misaligned pointer, n_rows < 1, n_nets outside {1, 2}, a wrong wstream_bytes and too
 * small a workspace return RISVEC_ERR_ARG; all are reported before anything is launched and without touching a device. */
typedef struct RisVecMarlCriticGradNet {
    RisVecMarlCriticNet fwd;
    const float *W2, *W3;
} RisVecMarlCriticGradNet;
typedef struct RisVecMarlCriticGrads {
    float *dW1, *db1, *dW2, *db2, *dW3, *db3, *dqw, *dqb;
} RisVecMarlCriticGrads;
int risvec_marl_critic_grad_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
size_t risvec_marl_critic_grad_workspace(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                         int32_t fc3, int32_t n_nets);
int risvec_marl_critic_grad(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                            int32_t n_nets, const RisVecMarlCriticGradNet *nets, const RisVecMarlCriticGrads *grads,
                            const float *state, const float *action, const float *target, float *q1, float *q2, float *loss,
                            void *workspace, size_t workspace_bytes, risvec_stream_t stream);
/* The critic side of the multi-agent (SAC) learner's actor update (Global_SAC_Critic.centralized_actor_update,
 * Simulation-MARL-BCD/global_sac_critic.py:174-176 and the backward() at :246): d min(q1, q2) / d action for n_rows rows and
 * n_nets in {1, 2} nets of one shape, without an autograd graph and without forming any weight gradient, in TWO launches on
 * `stream`, per row b and net c:
 *     d3 = qw [h3 > 0]   d2 = (W3^T d3) [h2 > 0]   d1 = (W2^T d2) [h1 > 0]   g_c[b, :] = (W1^T d1)[state_dims : state_dims + action_dims]
 *     w_1, w_2 = (1, 0) if q_1 < q_2, (0, 1) if q_1 > q_2, (0.5, 0.5) if q_1 == q_2  (torch.min's backward; n_nets == 1: w_1 = 1)
 *     out[b, :] = scale (w_1 g_1[b, :] + w_2 g_2[b, :])            q_min[b] = min(q_1[b], q_2[b])
 * Launch 1 (grid: 32-row tiles x nets) walks the forward of risvec_marl_critic on the packed stream (q_c has its bits), keeps
 * the ReLU masks as bits in registers, back-propagates the deltas within the workgroup -- the transposed products read the
 * float32 W1, W2 and W3 IN PLACE, scaled by the power of two that `scales` records and split on the fly; a tile's deltas are
 * multiplied by the exact power of two that brings its largest entry into [64, 128) and the accumulator is multiplied back --
 * and leaves g_c and q_c in the workspace.  No W1 column at or beyond state_dims + action_dims is read.  Launch 2 (one thread
 * per element of out) selects.  No atomics: every call gives the same bits.  No synchronisation, no allocation.
 *   nets[c].fwd    the net as risvec_marl_critic takes it: a stream that is current for W1, W2, W3;
 *   nets[c].W1 / W2 / W3  the float32 Linear weights [fc1, state_dims + action_dims] / [fc2, fc1] / [fc3, fc2] behind that
 *                  stream, float-aligned;
 *   state, action  as for risvec_marl_critic; no row >= n_rows is read;
 *   scale          multiplies out (the actor loss's -1 / n_rows, say);
 *   q1, q2 [n_rows]  optional: receive q_c; q2 with n_nets == 2 only;
 *   q_min [n_rows] optional;   out [n_rows, action_dims] required; rows >= n_rows of neither are written;
 *   workspace      risvec_marl_critic_action_grad_workspace(n_rows, ...) bytes (0: n_rows < 1, a shape that is not built, or
 *                  n_nets outside {1, 2}), 16-byte aligned, of any content.
 * Built for the shapes of risvec_marl_critic (risvec_marl_critic_action_grad_supported, host only); other shapes return
 * RISVEC_ERR_UNSUPPORTED.  A NULL or misaligned pointer, n_rows < 1, n_nets outside {1, 2}, a wrong wstream_bytes and too
 * small a workspace return RISVEC_ERR_ARG; all are reported before anything is launched and without touching a device. */
typedef struct RisVecMarlCriticActionGradNet {
    RisVecMarlCriticNet fwd;
    const float *W1, *W2, *W3;
} RisVecMarlCriticActionGradNet;
int risvec_marl_critic_action_grad_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3);
size_t risvec_marl_critic_action_grad_workspace(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1,
                                                int32_t fc2, int32_t fc3, int32_t n_nets);
int risvec_marl_critic_action_grad(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                   int32_t fc3, int32_t n_nets, const RisVecMarlCriticActionGradNet *nets, const float *state,
                                   const float *action, float scale, float *q1, float *q2, float *q_min, float *out,
                                   void *workspace, size_t workspace_bytes, risvec_stream_t stream);
/* Every agent's local twin target critics and local TD target of the multi-agent (SAC) learner (Agent.local_learn,
 * Simulation-MARL-BCD/sac_agent.py:263-284, called once per agent by global_sac_critic.py:373-392) in ONE launch for n_rows
 * rows and n_agents agents; grid (ceil(n_rows / 32), n_agents).  Agent j has n_nets in {1, 2} CriticNetworks of one shape
 * on [obs_j (state_dims) | action_j (action_dims)], nets[j n_nets + c] = its net c, each prepared exactly as a net of
 * risvec_marl_critic at (state_dims, action_dims) -- the same weight stream, built by the same pack -- and walked by the
 * same code:
 *     x   = [obs[row, j, 0:state_dims] | action_j]
 *     action_j = action[row, j, 0:action_dims]                               explicit form: `action` given
 *              = [onehot(idx) (n_agents) | power[row, j, 0:2]]               from the policy: `heads` and `power` given
 *         idx  = the FIRST maximum of heads[j, row, 4 + i], i < n_agents, after entry i == j is REPLACED by FLT_MAX / -2
 *                (sac_agent.py:270-272; it still wins where every other logit is lower; the lowest index wins a tie)
 *     q_c = the net's forward as in risvec_marl_critic;  m = n_nets == 2 ? min(q_1, q_2) : q_1
 *     t   = m - (coef[0] logp_power[row, j] + coef[1] logp_intent[row, j])   a term whose logp pointer is NULL is absent
 *     y[j, row] = reward[row, j] + ((1 - done[row]) gamma) t                 a PRODUCT, not a select, every operation
 *                 rounded on its own: a done row gives reward exactly for a finite t and NaN for an infinite one (:284)
 * obs [n_rows, n_agents, state_dims], action [n_rows, n_agents, action_dims], heads [n_agents, n_rows, 4 + n_agents] (the
 * policy's mu, log_std, intent logits), power [n_rows, n_agents, 2], reward, logp_power, logp_intent [n_rows, n_agents]
 * float32, done [n_rows] uint8 (0 / 1), coef [2] float32 ON THE DEVICE; done and coef are shared by the agents.  All are
 * read in place; the per-agent input never exists in memory.  q1, q2, y [n_agents, n_rows] are each optional (NULL: not
 * written), at least one must be given.  Exactly one of action / heads is given; heads needs power and action_dims ==
 * n_agents + 2; q2 needs n_nets == 2; y needs reward and done; a logp pointer needs coef and y.  nets is a HOST array of
 * n_agents * n_nets descriptors, copied into the kernel's argument block.  One launch on `stream`, nothing else.
 * Built for 1 <= n_agents <= 16 and the shapes of risvec_marl_critic at (state_dims, action_dims)
 * (risvec_local_critics_supported, host only); other shapes return RISVEC_ERR_UNSUPPORTED.  Every other argument error
 * returns RISVEC_ERR_ARG; all are reported before anything is launched and without touching a device.  NaN logits are not
 * supported. */
int risvec_local_critics_supported(int32_t n_agents, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                   int32_t fc3);
int risvec_local_critics(int32_t n_rows, int32_t n_agents, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                         int32_t fc3, int32_t n_nets, const RisVecMarlCriticNet *nets, const float *obs, const float *action,
                         const float *heads, const float *power, const float *reward, const uint8_t *done, float gamma,
                         const float *coef, const float *logp_power, const float *logp_intent, float *q1, float *q2, float *y,
                         risvec_stream_t stream);
/* The Polyak blend of update_network_parameters (Simulation-SARL/ddpg_torch.py:104-130) for n_tensors tensors in ONE
 * launch, in place:
 *     target[i][e] = fl32( fl32(tau * online[i][e]) + fl32(one_minus_tau * target[i][e]) )
 * two rounded products and one rounded sum, never a fused multiply-add: the bits of `tau * a + (1 - tau) * b` on
 * float32 tensors.  The caller passes one_minus_tau = (float)(1.0 - (double)tau), as that expression computes it.
 *   online, target, numel   HOST arrays of n_tensors entries (1 <= n_tensors <= 32), copied into the kernel's argument
 *                           block: device pointers to float32 data, float-aligned, and element counts >= 1.  A pair
 *                           whose pointers share their offset from a 16-byte boundary is blended 16 bytes at a time.
 * online[i] == target[i], a NULL entry, a misaligned pointer and a non-finite factor return RISVEC_ERR_ARG; n_tensors
 * or a numel out of range RISVEC_ERR_SHAPE -- all before any device is touched. */
int risvec_soft_update(int32_t n_tensors, const float *const *online, float *const *target, const int64_t *numel,
                       float tau, float one_minus_tau, risvec_stream_t stream);
int risvec_policy_heads(int32_t n_envs, int32_t n_veh, int32_t f2, int32_t n_heads, const float *g, const float *b2,
                        const float *ln_w, const float *ln_b, const float *Wh, const float *bh, float *heads,
                        risvec_stream_t stream);

/* ---- the optimiser step: clip_grad_norm_ -> torch.optim.Adam.step() -> the Polyak blend, for many networks ----------
 * A GROUP is one network: one clip_grad_norm_ scope and one torch.optim.Adam instance of the reference
 * (global_sac_critic.py:364-370 and :246-249, sac_agent.py:296-303).  One call serves n_groups groups over n_tensors
 * tensors in two launches (k_adam_sqsum, k_adam_step), or in one (k_adam_step) without RISVEC_ADAM_CLIP.  The
 * descriptors live in DEVICE memory that the caller owns, so neither count is bounded by a kernel's argument block; the
 * caller also passes the HOST arrays it uploaded them from, which is what this entry point checks.
 *
 * A workgroup owns one chunk of RISVEC_ADAM_CHUNK consecutive elements of one tensor.  Tensors are listed group by group
 * (tensors[i].group never decreases; every group has a tensor); tensors[i].first_block is the sum of
 * ceil(numel / RISVEC_ADAM_CHUNK) over the tensors before i, groups[g].first_block / n_blocks the range of group g, and
 * block_tensor[b] the tensor of workgroup b (n_blocks int32 in device memory).
 *
 * With RISVEC_ADAM_CLIP, partials[b] (n_blocks doubles) takes the sum of fl32(grad^2) over workgroup b's chunk, added up
 * in float64; every workgroup of k_adam_step then adds its group's partials in one fixed order, so the result is the
 * same bits in all of them and from run to run (no atomics), and
 *     norm = fl32(sqrt(sum))    coef = min(max_norm / (norm + 1e-6), 1)   in float32, NaN kept (error_if_nonfinite=False)
 * norms[g] = norm is clip_grad_norm_'s return value.  A group with max_norm < 0 is not clipped (coef = 1).  Per element,
 * every operation rounded to float32 on its own, never fused:
 *     g = grad * coef;  if (weight_decay != 0) g = g + weight_decay * param          (coupled L2 decay)
 *     m = m + (g - m) * fl32(1 - beta1)
 *     v = v * fl32(beta2) + (fl32(1 - beta2) * g) * g
 *     param = param - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 *     target = fl32(tau * param) + fl32(one_minus_tau * target)       with RISVEC_ADAM_BLEND, where target != NULL
 * step_size = fl32(lr / (1 - beta1^t)) and bc2_sqrt = fl32(sqrt(1 - beta2^t)), both formed in double.  `/` and sqrt are
 * correctly rounded.  With RISVEC_ADAM_WRITE_GRAD, grad * coef is written back as clip_grad_norm_ does in place.
 * A descriptor whose pointers all share their offset from a 16-byte boundary is served 16 bytes at a time.
 *
 * A NULL table, a table that is not 16-byte aligned, counts out of range, a block layout that does not follow from the
 * numels, a NULL / misaligned / aliased tensor pointer, non-finite lr / eps / tau, weight_decay < 0, beta1 / beta2
 * outside [0, 1), t < 1 and too small a workspace return RISVEC_ERR_ARG (counts: RISVEC_ERR_SHAPE), all before any
 * device is touched. */
#define RISVEC_ADAM_CHUNK 4096
enum { RISVEC_ADAM_CLIP = 1, RISVEC_ADAM_WRITE_GRAD = 2, RISVEC_ADAM_BLEND = 4 };
typedef struct RisVecAdamTensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    float *target;         /* may be NULL */
    int64_t numel;
    int32_t group;
    int32_t first_block;
    int64_t reserved;      /* 64 bytes */
} RisVecAdamTensor;
typedef struct RisVecAdamGroup {
    double lr;
    float weight_decay;
    float max_norm;        /* < 0: this group is not clipped */
    int32_t first_block;
    int32_t n_blocks;
    int64_t reserved;      /* 32 bytes */
} RisVecAdamGroup;
/* bytes of `partials` for a call of n_blocks workgroups (0 for n_blocks < 1) */
size_t risvec_adam_workspace(int32_t n_blocks);
int risvec_adam_step(int32_t n_tensors, int32_t n_groups, int32_t n_blocks, const RisVecAdamTensor *tensors,
                     const RisVecAdamGroup *groups, const int32_t *block_tensor, const RisVecAdamTensor *tensors_host,
                     const RisVecAdamGroup *groups_host, double beta1, double beta2, double eps, int64_t t, float tau,
                     float one_minus_tau, uint32_t flags, double *partials, size_t partials_bytes, float *norms,
                     risvec_stream_t stream);

/* ---- f4: the per-episode metrics sink --------------------------------------------------
 * The driver sums the `last_*` scalars, the clipped per-user rewards and the equivalent powers step by
 * step in Python floats and turns them into per-episode scalars for TensorBoard (marl_train_bcd.py,
 * TRAIN below: 1611-1662 accumulate, 1714 clip, 1717-1753 power, 1769 per-user sums, 1824 and 1838-1865
 * means, 1939-1941 min / var / Jain, 1927-2048 the tags).  Here every env keeps its own float64
 * accumulators on the device and the episode summary is reduced over the envs in two launches.
 *
 * acc [RISVEC_EP_FIXED + V, E] doubles (column-major: one row per quantity, envs contiguous), rows:
 *   0..13   sum over the episode's steps of metrics[slot]            (TRAIN:1626-1662)
 *   14      sum of sum_v power_w[0,v]  (offload, equivalent watts)    (TRAIN:1752)
 *   15      sum of sum_v power_w[1,v]  (local)                        (TRAIN:1753)
 *   16      max over the steps of the global reward (`ep_env_best`)   (TRAIN:1613-1622)
 *   17+v    sum of clip(reward_v, -user_clip, +user_clip)             (TRAIN:1714, 1769)            */
#define RISVEC_EP_FIXED 17
#define RISVEC_EP_COLS 21
enum {
    RISVEC_EP_GLOBAL_AVG = 0,      /* reward/global_avg            mean of the global reward       (1838) */
    RISVEC_EP_OFF_KBIT = 1,        /* traffic/offload_kbit_ep      SUM over the episode           (2047) */
    RISVEC_EP_LOCAL_KBIT = 2,      /* traffic/local_kbit_ep        SUM                            (2048) */
    RISVEC_EP_MEC_CYCLES = 3,      /* queue/mec_cycles             value after the LAST step      (1974) */
    RISVEC_EP_BACKLOG = 4,         /* queue/backlog_kbit_ep_mean                                  (1862) */
    RISVEC_EP_DELAY_LOCAL = 5,     /* delay/local_ep_mean                                         (1858) */
    RISVEC_EP_DELAY_EDGE_Q = 6,    /* delay/edge_queue_ep_mean                                    (1859) */
    RISVEC_EP_DELAY_EDGE_C = 7,    /* delay/edge_compute_ep_mean                                  (1860) */
    RISVEC_EP_DELAY_TX = 8,        /* delay/tx_ep_mean                                            (1861) */
    RISVEC_EP_MEC_UTIL = 9,        /* queue/mec_util_ep_mean                                      (1863) */
    RISVEC_EP_LOCAL_UTIL = 10,     /* cpu/local_util_ep_mean                                      (1864) */
    RISVEC_EP_QOS_VIOL = 11,       /* qos/violation_rate_ep_mean                                  (1865) */
    RISVEC_EP_DELAY = 12,          /* delay/episode_mean  (abs/delay_ms = 1000 x this)            (1850) */
    RISVEC_EP_ENERGY = 13,         /* energy/episode_mean (abs/energy_J)                          (1851) */
    RISVEC_EP_POWER_OFFLOAD = 14,  /* power/offload_avg                                           (1843) */
    RISVEC_EP_POWER_LOCAL = 15,    /* power/local_avg                                             (1842) */
    RISVEC_EP_POWER_TOTAL = 16,    /* power/total_avg                                             (1841) */
    RISVEC_EP_MIN_USER = 17,       /* min over users of the per-user episode mean                 (1939) */
    RISVEC_EP_VAR_USER = 18,       /* population variance of the same                             (1940) */
    RISVEC_EP_JAIN = 19,           /* (sum x)^2 / (V sum x^2 + 1e-12)                         (112-119) */
    RISVEC_EP_BEST_GLOBAL = 20     /* best global reward of the episode                           (1613) */
};

/* Zero acc (column 16 to -inf).  Call where the driver resets its ep_* sums (TRAIN:1278-1300). */
int risvec_episode_clear(int32_t n_envs, int32_t n_veh, double *acc, risvec_stream_t stream);

/* One step's contribution: metrics [E,16] and reward [E,V] as the step kernel wrote them, power_w
 * [E,2,V] or NULL (then columns 14/15 stay untouched, as when the env has no last_power_W). */
int risvec_episode_accumulate(int32_t n_envs, int32_t n_veh, const float *metrics, const float *reward,
                              const float *power_w, float user_clip, double *acc, risvec_stream_t stream);

/* Episode end.  per_env [E, RISVEC_EP_COLS] (optional) receives every env's episode scalars; summary
 * [3, RISVEC_EP_COLS] their mean / min / max over the envs, reduced in a fixed order (deterministic);
 * partial is scratch of risvec_episode_partial_rows(n_envs) x 3 x RISVEC_EP_COLS doubles.  n_steps
 * >= 1; metrics supplies column 3 (the queue after the last step). */
int32_t risvec_episode_partial_rows(int32_t n_envs);
int risvec_episode_summary(int32_t n_envs, int32_t n_veh, int32_t n_steps, const double *acc, const float *metrics,
                           double *per_env, double *partial, double *summary, risvec_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RISVEC_H */
