/*
 * booster_gym_amd.h -- C ABI of libbooster_gym_amd.so (MI355X / gfx950, HIP).
 *
 * Drop-in boundary for the hot path of Nyro-Robotics/booster_gym: the Isaac Gym
 * tensor API the reference's task code calls plus the
 * GAE / PPO-loss loop of utils/runner.py.  Every entry point is extern "C",
 * takes plain pointers and sizes (device pointers are raw `void*` from
 * `torch.Tensor.data_ptr()`), returns 0 on success and a negative code on error
 * (`bg_last_error()` returns a thread-local message).  No function synchronises
 * the device or allocates after create; all work is enqueued on the caller's
 * `stream` (a hipStream_t passed as void*, NULL = default stream).
 *
 * Citations `file:line` refer to the reference tree.
 */
#ifndef BOOSTER_GYM_AMD_H
#define BOOSTER_GYM_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_NUM_BODIES 13
#define BG_NUM_DOFS 12
#define BG_NUM_OBS 47
#define BG_NUM_PRIV 14
#define BG_NUM_REWARD_TERMS 26
#define BG_MAX_BODY_SPHERES 16
#define BG_MAX_HEIGHT_SCAN_POINTS 1024 /* bg_env_cfg.height_scan_points */
#define BG_ACTOR_MAX_INPUT 480 /* bg_actor_sample_mlp: the widest first layer (47 H observations + P height-scan values), ten 48-column k-chunks */
#define BG_MAX_FRAME_STACK 10 /* bg_env_cfg.frame_stack: 47 x 10 = 470 observation columns, within the 512 of the widest first layer */

typedef struct bg_model bg_model;
typedef struct bg_env bg_env;

/* Flat articulated-body model (what Isaac Gym's load_asset + asset queries return:
 * envs/t1.py:54-67, 85-108).  Bodies depth-first: trunk, left leg 1..6, right leg 7..12. */
typedef struct {
    int32_t num_bodies, num_dofs;
    int32_t parent[BG_NUM_BODIES];
    int32_t joint_axis[BG_NUM_BODIES]; /* 0 floating base, 1/2/3 revolute about x/y/z */
    float body_pos[BG_NUM_BODIES][3];
    float mass[BG_NUM_BODIES];
    float com[BG_NUM_BODIES][3];
    float inertia[BG_NUM_BODIES][6]; /* about com: xx yy zz xy xz yz */
    float dof_lower[BG_NUM_DOFS], dof_upper[BG_NUM_DOFS], dof_velocity[BG_NUM_DOFS], dof_effort[BG_NUM_DOFS];
    float feet_edge_pos[4][3]; /* cfg asset.feet_edge_pos, envs/T1.yaml:79-82 */
    /* contact spheres of the NON-foot collision shapes of the asset (URDF <collision>: box corners with radius 0, two spheres inscribed in the
     * ends of a cylinder), sorted by body; bodies are the trunk or leg links.  num_body_spheres = 0 switches these contacts off. */
    int32_t num_body_spheres;
    int32_t sphere_body[BG_MAX_BODY_SPHERES];
    float sphere_pos[BG_MAX_BODY_SPHERES][3];
    float sphere_radius[BG_MAX_BODY_SPHERES];
    /* Self-collision capsules (gym.create_actor(..., self_collisions), envs/t1.py:128; asset.self_collisions, envs/T1.yaml:69): [leg][0] the shank
     * (4th link of the leg chain; the capsule inscribed in its URDF cylinder, axis z), [leg][1] the foot (last link; a capsule along x standing in
     * for the URDF box).  Segment end points a / b in link coordinates and the radius; radius 0 on any of them = the model has no self-collision
     * geometry.  Left-leg capsules meet right-leg capsules; links of one chain never meet each other. */
    float self_capsule_a[2][2][3], self_capsule_b[2][2][3], self_capsule_r[2][2];
} bg_model_desc;

/* randomisation / noise entry (utils/utils.py:5-30): mode 0 none, 1 gaussian additive,
 * 2 gaussian scaling, 3 uniform additive, 4 uniform scaling; (a,b) = the yaml `range`. */
typedef struct { int32_t mode; float a, b; } bg_rand;

/* order of reward terms = order of envs/T1.yaml:252-278; scale 0 drops the term (t1.py:280-285) */
enum {
    BG_REW_SURVIVAL = 0, BG_REW_TRACKING_LIN_VEL_X, BG_REW_TRACKING_LIN_VEL_Y, BG_REW_TRACKING_ANG_VEL, BG_REW_BASE_HEIGHT,
    BG_REW_ORIENTATION, BG_REW_TORQUES, BG_REW_TORQUE_TIREDNESS, BG_REW_POWER, BG_REW_LIN_VEL_Z, BG_REW_ANG_VEL_XY, BG_REW_DOF_VEL,
    BG_REW_DOF_ACC, BG_REW_ROOT_ACC, BG_REW_ACTION_RATE, BG_REW_DOF_POS_LIMITS, BG_REW_DOF_VEL_LIMITS, BG_REW_TORQUE_LIMITS,
    BG_REW_COLLISION, BG_REW_FEET_SLIP, BG_REW_FEET_VEL_Z, BG_REW_FEET_YAW_DIFF, BG_REW_FEET_YAW_MEAN, BG_REW_FEET_ROLL,
    BG_REW_FEET_DISTANCE, BG_REW_FEET_SWING
};

/* Everything numeric the env needs from envs/T1.yaml (sections sim, control, normalization,
 * noise, randomization, commands, rewards, init_state, terrain) plus this build's contact model. */
typedef struct {
    int32_t num_envs;
    int32_t device;     /* HIP device ordinal; there is no CPU path in this library */
    uint64_t seed;
    /* sim (T1.yaml:39-44) + contact model of this build */
    float sim_dt;
    int32_t decimation; /* control.decimation, T1.yaml:95 */
    float gravity[3];
    float contact_k, contact_d, contact_ramp, friction_visc, limit_k, limit_d;
    float terrain_mu, terrain_restitution; /* T1.yaml:99-101 */
    int32_t clamp_qd;
    /* control / normalization (T1.yaml:91-95, 135-145) */
    float action_scale, clip_actions;
    float norm_gravity, norm_lin_vel, norm_ang_vel, norm_dof_pos, norm_dof_vel, filter_weight, norm_push_force, norm_push_torque;
    float default_dof_pos[BG_NUM_DOFS]; /* t1.py:264-272 */
    float base_init_state[13];          /* t1.py:109-112 */
    /* noise (T1.yaml:147-171) */
    bg_rand noise_gravity, noise_lin_vel, noise_ang_vel, noise_dof_pos, noise_dof_vel, noise_height;
    /* run-time randomisation (T1.yaml:173-206) */
    bg_rand init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy, kick_lin_vel, kick_ang_vel, push_force, push_torque;
    int32_t kick_interval, push_interval, push_duration; /* in env steps: ceil(seconds / dt), t1.py:501,508,517 */
    int32_t shared_reset_noise; /* 1 = reference quirk Q1 (t1.py:320): one noise vector per reset call */
    /* commands (T1.yaml:115-133) */
    float cmd_lin_vel_x[2], cmd_lin_vel_y[2], cmd_ang_vel_yaw[2], cmd_gait_frequency[2];
    float still_proportion;
    int32_t resample_steps[2]; /* int(seconds / dt), t1.py:384-385 */
    /* command curriculum (T1.yaml:124-133, t1.py:391-435); levels are +-lin_vel_levels x +-ang_vel_levels */
    int32_t curriculum;
    int32_t lin_vel_levels, ang_vel_levels;
    float curriculum_update_rate, lin_vel_x_resolution, lin_vel_y_resolution, ang_vel_resolution;
    float episode_length_toler, lin_vel_x_toler, lin_vel_y_toler, ang_vel_yaw_toler;
    /* rewards (T1.yaml:251-291) */
    float reward_scale[BG_NUM_REWARD_TERMS]; /* yaml value * dt; 0 = dropped */
    int32_t only_positive_rewards;
    float tracking_sigma, base_height_target, soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit, swing_period, feet_distance_ref;
    int32_t max_episode_length; /* ceil(episode_length_s / dt), t1.py:556 */
    float terminate_height, terminate_vel;
    /* terrain extents for the teleport wrap (t1.py:343-360); plane => teleport off */
    int32_t terrain_type; /* 0 plane, 1 heightfield ("trimesh" in the yaml) */
    float terrain_env_width, terrain_env_length, terrain_border;
    /* 1 = keep the per-env dynamic state in fp16 between env steps (BASELINE.json configs[4]; T1.yaml sim.state_dtype: fp16): orientation,
     * velocities, joint state, targets / actions and their histories, commands, gait, filters, push wrench.  Arithmetic stays fp32; root position,
     * last feet positions, parameters and outputs stay fp32.  bg_env_get/set_state / get/set_field convert transparently. */
    int32_t state_fp16;
    /* non-foot body contacts: evaluated for envs whose trunk origin starts the step lower than body_gate_height above
     * the terrain, and only if body_gate_height > terminate_height (otherwise every such env has been reset before its next step and the
     * second launch that handles them is left out altogether).
     * Bit b of the masks = body b: rewards.penalize_contacts_on / terminate_contacts_on resolved against the body names (t1.py:85-100);
     * a body counts when its net contact force exceeds 1 N (t1.py:553,629). */
    float body_gate_height;
    int32_t penalized_body_mask, terminate_body_mask;
    /* Reference-exact command resampling (T1.yaml parallel.exact_still_count / parallel.same_step_curriculum; default 0 = this build's
     * single-launch forms).  exact_still_count: exactly int(still_proportion * K) of the K envs that resample in a step stand still, a uniformly
     * random subset (t1.py:381-383 randperm prefix) instead of a per-env Bernoulli draw.  same_step_curriculum: the curriculum sampler reads the
     * grid AFTER this step's resets have updated it (t1.py:305 before :365) instead of the grid as of the start of the step.  Either one moves
     * the cross-env part of _resample_commands into two small follow-up launches per env step (count, apply); not available with state_fp16. */
    int32_t exact_still_count, same_step_curriculum;
    /* Leg-against-leg contacts (asset.self_collisions: 0 in envs/T1.yaml:69 is Isaac Gym's "collide with everything", passed to create_actor at
     * envs/t1.py:128): 1 = the shank / foot capsules of the two legs repel each other with an explicit penalty force:
     * normal stiffness [N/m] and damping [N s/m], Coulomb coefficient, and the viscous cap [N s/m] of the regularised friction. */
    int32_t self_collisions;
    float self_k, self_d, self_mu, self_visc;
    /* Terrain curriculum (T1.yaml terrain.curriculum; an addition of this build, legged_gym's rule).  0 = off: nothing below is read and no
     * per-env level is kept.  1 = the height field holds terrain_num_levels rows of terrain_tile_length along y (difficulty (l + 1) / levels)
     * by the type columns of terrain_tile_width along x; every env has a level and a fixed column, and at each reset of an env step (not
     * bg_env_reset) its level moves up when the robot walked farther than terrain_tile_length / 2 from its origin, down when it walked less than
     * |command xy| * terrain_down_time (rewards.episode_length_s / 2), wraps to a random level past the top, and the origin becomes the centre
     * of the env's new tile.  Levels / columns: fields "terrain_level" / "terrain_type"; their running sum: bg_env_get/set_terrain_level_sum. */
    int32_t terrain_curriculum, terrain_num_levels;
    float terrain_tile_width, terrain_tile_length, terrain_down_time;
    /* Terrain height scan of the critic (T1.yaml terrain.measure_heights; an addition of this build, legged_gym's measured heights).  0 points =
     * off: nothing below is read and the privileged row is the 14 values.  P > 0 (a height field only): after every env step and reset-all, one
     * more launch (bg_height_scan) writes columns 14 .. 14 + P of each privileged row [N][14 + P] ([N][14 + P + X] with priv_extras, below):
     *   clip(base z - h(base xy + Rz(yaw) (x_p, y_p)) - base_height_target, -1, 1) * height_scan_scale
     * with h the bilinear ground height, yaw that of the stored base quaternion, no noise. */
    int32_t height_scan_points;       /* P: points of the scan (0 = off) */
    const float* height_scan_xy;      /* host float [P][2]: (x, y) of each point in the robot's yaw frame [m]; copied by bg_env_create */
    float height_scan_scale;          /* normalization.height_measurements */
    /* Observation history of the actor's input (T1.yaml env.frame_stack; an addition of this build, humanoid-gym's frame_stack).  H = 1, or 0 (a
     * zero-initialised struct: every caller older than the field), is no history: the observation output is [N][47] and no launch is added.
     * H in 2 .. BG_MAX_FRAME_STACK: the observation output (bound or passed to bg_env_step_to) is [N][47 H], the last H single observations of
     * each env oldest first, newest last; the env keeps the history itself and one more launch (bg_obs_stack) behind every env step and
     * reset-all writes the row.  An env that was reset in the step (every env, for bg_env_reset) gets H - 1 zero frames and its new observation.
     * Negative or above BG_MAX_FRAME_STACK: bg_env_create fails. */
    int32_t frame_stack;
    /* Terrain height scan in the actor's input (T1.yaml terrain.actor_heights; an addition of this build, legged_gym's perceptive policy).  0 = off:
     * nothing below is read and every launch is as without the field.  1 (height_scan_points = P > 0 only, else bg_env_create fails): the observation
     * output (bound or passed to bg_env_step_to) is [N][47 H + P]: the H single observations as with frame_stack (H = 1 included), then once, not
     * stacked, the newest scan with noise:
     *   clip(base z - h_p - base_height_target, -1, 1) * height_scan_scale + height_scan_scale * n_p,
     * n_p [m] = apply_rand(0, noise_height_measurements, u, n) on entry p & 3 of Philox(seed, env, step count, RS_SCAN + (p >> 2)) (RS_SCAN_RESET at
     * bg_env_reset; csrc/bg_rng.h).  The privileged columns 14 .. 14 + P keep the clean scan, bit for bit the first term.  One launch
     * (bg_obs_assemble), the last of every env step and reset-all, writes both and takes the place of bg_height_scan and bg_obs_stack; the env keeps
     * its ring of H observation planes also at H = 1.  num_envs x (47 H + P) must stay below 2^31. */
    int32_t actor_heights;
    bg_rand noise_height_measurements; /* noise.height_measurements [m]; read with actor_heights only */
    /* A longer observation history for the student of a distillation (T1.yaml distillation.student_frame_stack; utils/distill.py).  0 = off: nothing
     * changes (a zero-initialised struct: every caller older than the field).  Hs in frame_stack .. BG_MAX_FRAME_STACK, with actor_heights only (else
     * bg_env_create fails): the env's ring has Hs planes and bg_obs_assemble, still the one and last launch of every env step and reset-all, writes a
     * third output, the student's row [N][47 Hs]: the env's last Hs single observations oldest first, newest last, frames from before the env's last
     * reset zero (frame_stack's rule at Hs frames).  Its last 47 H columns are the first 47 H columns of the actor's row [47 H + P], noise included.
     * The destination comes from bg_env_bind_student_obs (bg_env_reset, bg_env_step) or bg_env_step_to_student; a reset or step without one is an
     * error, and so is bg_env_step_to.  num_envs x 47 Hs must stay below 2^31. */
    int32_t student_frame_stack;
    /* More of what the env randomises and computes, for the critic (T1.yaml env.privileged_extras; an addition of this build, humanoid-gym's
     * env_frictions / contact_mask and the foot height / contact targets of Ji et al. 2022).  priv_extras = 0 = off (a zero-initialised struct: every
     * caller older than the field): nothing below is read and no launch is added.  Otherwise a bitmask of BG_PRIV_EXTRA_*; the privileged row is
     * [N][14 + P + X] and one more launch (bg_priv_extras) behind the env-step kernels of every env step and reset-all, in front of bg_height_scan /
     * bg_obs_stack / bg_obs_assemble, writes its columns [14 + P, 14 + P + X), the groups in the fixed order feet, ground, joints (left foot = leg 0
     * first), all from the STORED per-env fields (bg_env_get_field's names), without noise:
     *   FEET (6):    feet_contact[0], [1];  clip(feet_contact_forces[leg][z] * priv_force_scale, -5, 5) of leg 0, 1;
     *                clip(feet_pos[leg][z] - h(feet_pos[leg][xy]), -1, 1) * priv_clearance_scale of leg 0, 1, h the bilinear ground height (0 on a plane)
     *   GROUND (6):  foot_material[0..6) = friction, compliance, restitution of the left foot, then of the right
     *   JOINTS (12): dof_friction[0..12)
     * On the step in which an env resets, the feet fields are those the env step stored BEFORE the reset pose (the reference's buffers of the same
     * names behave so), while the root and the 14 columns are the new episode's.  An unknown bit or num_envs x (14 + P + X) >= 2^31: bg_env_create fails. */
    int32_t priv_extras;
    float priv_force_scale;     /* normalization.contact_force; read with BG_PRIV_EXTRA_FEET only */
    float priv_clearance_scale; /* normalization.height_measurements; read with BG_PRIV_EXTRA_FEET only */
    /* Sensor model of the actor's row (T1.yaml sensors; an addition of this build, IsaacLab's NoiseModelWithAdditiveBias and a sensing delay).
     * sensor_model = 0 = off (a zero-initialised struct: every caller older than the field): nothing below is read and every launch is as without it.
     * 1 (not with actor_heights, else bg_env_create fails): the env keeps a ring of frame_stack + ceil(sensor_latency_hi) single observations, also
     * at frame_stack 1, and one launch (bg_obs_sensor), the last of every env step and reset-all, in the place of bg_obs_stack, writes the actor's row
     * [N][47 H].  With age = the env steps since the env's last reset (0 on the step that reset it; the field "episode_length_buf") and o(j) the stored
     * single observation of j steps ago, frame k (d = H - 1 - k steps ago) is zero when d > age (bg_obs_stack's reset rule), else o(d) in every column
     * but the 30 sensor columns (gravity 0-2, angular velocity 3-5, dof_pos 11-22, dof_vel 23-34; sensor column s = c for c < 6, c - 5 otherwise), which
     * are, with i = floor(lam), f = lam - i, a = o(min(d + i, age)), b = o(min(d + i + 1, age)):  a + f (b - a) + beta[s]  in fp32.  The interpolation
     * is left out when sensor_latency_lo = sensor_latency_hi = 0 (and b is not read where f = 0), the add for a group whose sensor_bias_* has mode 0.
     * On the step that resets an env (every env, for bg_env_reset) the launch draws and stores, until the env's next reset,
     *   beta[s] = apply_rand(0, sensor_bias_<group of s>, u, n) * norm_<group>  on entry s & 3 of Philox(seed, env, step count, RS_SENSOR + (s >> 2)),
     *   lam     = sensor_latency_lo + (sensor_latency_hi - sensor_latency_lo) * u  on entry 0 of stream RS_SENSOR + 8
     * (RS_SENSOR_RESET at bg_env_reset; csrc/bg_rng.h).  Fields "sensor_bias" [N][30] and "sensor_latency" [N] read them back (bg_env_get_field only).
     * The env-step kernels, the privileged row and every other stream are untouched.  sensor_bias_*: mode 0 (none), 1 (gaussian additive: a = mean,
     * b = std >= 0) or 3 (uniform additive: a = low, b = high), finite; 0 <= sensor_latency_lo <= sensor_latency_hi <= BG_MAX_SENSOR_LATENCY.
     * 2 = the student's row only (T1.yaml distillation.student_sensors; with actor_heights and student_frame_stack = Hs >= 1 only, else bg_env_create
     * fails): the actor's row [47 H + P] and the privileged row stay bit for bit what they are at 0, and the student's row [N][47 Hs], the third
     * output of bg_obs_assemble, follows the rule above at Hs frames, with the draws above on the same streams: it has the bits of the actor's row of
     * an env with sensor_model = 1, frame_stack = Hs and the same seed.  The ring has Hs + ceil(sensor_latency_hi) planes, bg_obs_assemble stays
     * the one and last launch of every env step and reset-all and does not write the ring, bg_obs_sensor never runs (bg_env_sensor_launches stays 0),
     * and the two fields are readable as with 1.  The sensor_bias_* and sensor_latency_* fields and their ranges are the same; no field is added. */
    int32_t sensor_model;
    bg_rand sensor_bias_gravity, sensor_bias_ang_vel, sensor_bias_dof_pos, sensor_bias_dof_vel; /* sensors.bias.*, in physical units */
    float sensor_latency_lo, sensor_latency_hi;                                                 /* sensors.latency_steps, in env steps */
} bg_env_cfg;
#define BG_NUM_SENSOR_COLS 30    /* columns of the field "sensor_bias" */
#define BG_MAX_SENSOR_LATENCY 2  /* the most of sensor_latency_hi */
#define BG_PRIV_EXTRA_FEET 1
#define BG_PRIV_EXTRA_GROUND 2
#define BG_PRIV_EXTRA_JOINTS 4
#define BG_PRIV_EXTRA_ALL 7

/* ---- model (replaces gym.load_asset and the asset queries, t1.py:54-108) */
int bg_model_create(const bg_model_desc* desc, bg_model** out);
/* gym.load_asset(sim, root, file, asset_options) with collapse_fixed_joints (envs/t1.py:39-54, envs/T1.yaml:61-83) for hosts without the Python
 * loader: parses the URDF at `path`, folds links behind fixed joints into their parents (masses, centres of mass, inertias, collision
 * primitives), orders bodies / DoFs depth-first like Isaac Gym and fills the flat model, including the contact spheres of the non-foot
 * collision primitives.  foot_names = cfg asset.foot_names (their boxes are the sole-corner contacts, not spheres), feet_edge_pos = cfg
 * asset.feet_edge_pos.  The same algorithm as booster_gym_amd/utils/urdf.py (tests/test_host_logic.py compares the two on the same files). */
typedef struct {
    int32_t collapse_fixed_joints;  /* envs/T1.yaml:67 */
    int32_t body_contacts;          /* 0: no contact spheres (feet-only contact) */
    int32_t self_collisions;        /* 0: no self-collision capsules */
    const char* foot_names[2];      /* envs/T1.yaml:78 */
    float feet_edge_pos[4][3];      /* envs/T1.yaml:79-82 */
} bg_asset_options;
int bg_model_load_urdf(const char* path, const bg_asset_options* options, bg_model** out);
/* gym.get_asset_rigid_body_names / get_asset_dof_names / find_asset_rigid_body_index (t1.py:57,85,92-106); NULL / -1 when out of range or
 * when the model was made by bg_model_create (no names).  Counts, limits and efforts (t1.py:55-67): bg_model_get. */
const char* bg_model_body_name(const bg_model* m, int32_t i);
const char* bg_model_dof_name(const bg_model* m, int32_t j);
int32_t bg_model_find_body(const bg_model* m, const char* name);
int bg_model_get(const bg_model* m, bg_model_desc* out);
void bg_model_destroy(bg_model* m);

/* ---- env = simulator + T1 task logic (replaces create_sim/create_env/create_actor/prepare_sim,
 *      base_task.py:20-79, t1.py:33-137, and owns the per-env state of t1.py:187-272) */
int bg_env_create(const bg_env_cfg* cfg, const bg_model* model, bg_env** out);
void bg_env_destroy(bg_env* env);
/* height field for terrain.type "trimesh" (utils/terrain.py:30-99): host int16 [rows][cols], copied to the device */
int bg_env_set_heightfield(bg_env* env, const int16_t* hf_host, int32_t rows, int32_t cols, int32_t border_px, float hscale, float vscale);
/* per-env build-time randomisation (t1.py:69-83, 122-167), host float arrays, env-major:
 * kp/kd/friction [N][12], mass_scale [N][13], com_offset [N][13][3], foot_material [N][2][3] = (friction, compliance,
 * restitution), base_mass_scaled [N][4] (raw draws shown to the critic, t1.py:141-152), env_origins [N][3] (t1.py:169-185) */
int bg_env_set_params(bg_env* env, const float* kp, const float* kd, const float* friction, const float* mass_scale, const float* com_offset,
                      const float* foot_material, const float* base_mass_scaled, const float* env_origins);
/* outputs of reset/step, device pointers owned by the caller (torch tensors): obs [N][47 H] (H = cfg.frame_stack, [N][47] without a
 * history; [N][47 H + P] with cfg.actor_heights), privileged [N][14 + P + X] (P = cfg.height_scan_points, 0 without the height scan; X = the columns of cfg.priv_extras, 0 without: [N][14]), rew [N], done uint8 [N], time_outs uint8 [N], rew_terms [26][N] (rows of dropped terms stay 0) */
int bg_env_bind_outputs(bg_env* env, float* obs, float* privileged_obs, float* rew, uint8_t* done, uint8_t* time_outs, float* rew_terms);
/* The student's row of bg_env_reset / bg_env_step (bg_env_cfg.student_frame_stack = Hs): device float [N][47 Hs], owned by the caller.  An error
 * naming the field when it is 0. */
int bg_env_bind_student_obs(bg_env* env, float* student_obs);
/* T1.reset(): t1.py:294-299 */
int bg_env_reset(bg_env* env, void* stream);
/* T1.step(actions): t1.py:437-497.  actions: device float [N][12] */
int bg_env_step(bg_env* env, const float* actions, void* stream);
/* Same, writing obs/privileged/rew/done/time_outs of this step to the given device pointers instead of
 * the bound ones (lets the rollout loop write straight into rows of the experience buffer, runner.py:107-118) */
int bg_env_step_to(bg_env* env, const float* actions, float* obs, float* privileged_obs, float* rew, uint8_t* done, uint8_t* time_outs,
                   void* stream);
/* bg_env_step_to with the student's row [N][47 Hs] of this step (bg_env_cfg.student_frame_stack; an error naming the field when it is 0) */
int bg_env_step_to_student(bg_env* env, const float* actions, float* obs, float* privileged_obs, float* rew, uint8_t* done, uint8_t* time_outs,
                           float* student_obs, void* stream);
/* Isaac-Gym-layout views of the simulator state for inspection / tests (device pointers, may be NULL):
 * root [N][13] (pos, quat xyzw, lin vel, ang vel: t1.py:215), dof [N][12][2] (pos, vel: t1.py:216-218),
 * contact [N][13][3] net contact force per body, world frame (t1.py:219) */
int bg_env_get_state(bg_env* env, float* root, float* dof, float* contact, void* stream);
int bg_env_set_state(bg_env* env, const float* root, const float* dof, void* stream);
/* named per-env arrays (task state of t1.py:187-272), float or int32 depending on the field; see bg_env_field_info */
int bg_env_get_field(bg_env* env, const char* name, void* dst_device, void* stream);
int bg_env_set_field(bg_env* env, const char* name, const void* src_device, void* stream);
int bg_env_field_info(bg_env* env, const char* name, int32_t* components, int32_t* is_int);
/* curriculum_prob grid [(2*lin_vel_levels+1)][(2*ang_vel_levels+1)] (t1.py:249-255), device float pointers.  The library keeps the
 * UNCLAMPED running sums (increments are positive, so min(sum, 1) equals the reference's clamp_(max=1) after every update);
 * get returns min(sum, 1). */
int bg_env_get_curriculum(bg_env* env, float* prob_device, void* stream);
int bg_env_set_curriculum(bg_env* env, const float* prob_device, void* stream);
/* terrain curriculum (cfg.terrain_curriculum = 1 only, else -1): the sum of all envs' levels, one int32 at a device pointer, kept by the env
 * step's resets with one atomic add per change (no reduction launch).  The setter is for restores that write "terrain_level" directly. */
int bg_env_get_terrain_level_sum(bg_env* env, int32_t* sum_device, void* stream);
int bg_env_set_terrain_level_sum(bg_env* env, const int32_t* sum_device, void* stream);
int64_t bg_env_step_count(const bg_env* env);
int bg_env_set_step_count(bg_env* env, int64_t count);
/* bg_obs_sensor launches this env has enqueued since bg_env_create (cfg.sensor_model: one per env step and per reset-all; 0 for ever with the
 * model off), -1 for a null env.  A host counter, for tests and tools that must know which launch wrote the actor's row. */
int64_t bg_env_sensor_launches(const bg_env* env);
/* ---- evaluation record: per-robot metrics of every env's FIRST episode, kept by one launch after each env step (evaluate.py).  Not part of
 * bg_env_step's launch sequence: a training run that never calls these launches nothing new.  `record` is the caller's device float
 * [BG_EVAL_PLANES][N], plane-major (a wave's loads and stores are contiguous):
 *   0 STATE (0 running, 1 ended by the time-out, 2 ended by a termination)   1 LEN   2 REW   3 LEVEL   4 TYPE (terrain level and column, 0 / 0
 *   without cfg.terrain_curriculum)   5, 6 X0, Y0   7, 8 X1, Y1   9 CLASS   10 POWER   11 + 4 c + {0, 1, 2, 3}: CNT, SQ_vx, SQ_vy, SQ_yaw of the
 *   command class c = 0 (every |cmd_a| <= 1e-6), 1 (max |cmd_a| <= 0.5), 2 (the rest).
 * begin is called after bg_env_reset, step after every env step with the rew / done / time_outs (uint8) that step wrote; settle_steps: the steps
 * at the start of an episode that give no tracking sample.  The rule of both is stated once, at the kernel (bg_eval_step, csrc/bg_sim.hip), and
 * once for users, in the README's evaluation paragraph.
 * A null env / record / rew / done / time_outs or a negative settle_steps is -1 naming the argument, before anything is launched. */
#define BG_EVAL_PLANES 23
int bg_env_eval_begin(bg_env* env, float* record, void* stream);
int bg_env_eval_step(bg_env* env, const float* rew, const uint8_t* done, const uint8_t* time_outs, int32_t settle_steps, float* record,
                     void* stream);
/* ---- gait record: a second, opt-in per-robot record of every env's FIRST episode (evaluate.py --gait): action smoothness, effort, body wobble,
 * duty factor, touchdowns, slip, swing clearance.  The conventions are the evaluation record's: the caller's device float [BG_GAIT_PLANES][N],
 * plane-major, one launch per call, no bg_env_cfg field, not part of bg_env_step's launch sequence.  It is independent of the evaluation record (its
 * own STATE and LEN planes: either step may be called first).  Planes (foot f = 0 left, 1 right):
 *   0 STATE (0 running, 1 ended)  1 LEN  2 MOV  3 D1  4 D2  5 TAU2  6 TILT  7 WOBBLE  8 DS  9 FL
 *   10 + 2 k + f, k = 0 .. 7: STANCE, TD, IMP, PEAK, SLIP, CLR, SWT, SWC of foot f
 *   carries: 26 .. 37 A1[12]  38 .. 49 A2[12]  50, 51 CPREV[f]  52 + 2 f + {0, 1} PPREV[f].xy  56, 57 SWMAX[f]  58, 59 SWN[f]
 * The rule (stated once more at the kernel, bg_gait_step in csrc/bg_sim.hip, and for users in the README's evaluation paragraph), from the fields the
 * env step has stored: a actions, tau torques, g projected_gravity, w base_ang_vel, cmd commands, c_f = feet_contact[f] > 0.5, Fz_f =
 * feet_contact_forces[3 f + 2], p_f = feet_pos[3 f ..], clr_f = p_f.z - terrain height under p_f.xy (0 on a plane):
 *   begin (after bg_env_reset): every plane 0.
 *   step (after an env step that wrote `done`):  STATE != 0: nothing of the env is written.  LEN += 1 (len = the new value).  done: STATE = 1, no sample.
 *     Otherwise  TAU2 += sum tau_j^2, TILT += g.x^2 + g.y^2, WOBBLE += w.x^2 + w.y^2, PEAK_f = max(PEAK_f, Fz_f);
 *     len >= 2: D1 += sum (a_j - A1_j)^2;  len >= 3: D2 += sum (a_j - 2 A1_j + A2_j)^2;
 *     !c_f: SWMAX_f = SWN_f == 0 ? clr_f : max(SWMAX_f, clr_f), SWN_f += 1;
 *     moving = len > settle_steps and max |cmd_a| > 1e-6:  MOV += 1, STANCE_f += c_f, DS += c_0 and c_1, FL += neither;
 *         touchdown (len >= 2, c_f, not CPREV_f): TD_f += 1, IMP_f += Fz_f, and with SWN_f > 0: CLR_f += SWMAX_f, SWT_f += SWN_f, SWC_f += 1;
 *         stance (len >= 2, c_f, CPREV_f): d = |p_f.xy - PPREV_f|, SLIP_f += d where d <= 0.5 (a larger jump is the terrain's teleport wrap);
 *     c_f: SWN_f = SWMAX_f = 0;  then A2 = A1, A1 = a, CPREV_f = c_f, PPREV_f = p_f.xy.
 * A null env / record / done or a negative settle_steps is -1 naming the argument, before anything is launched. */
#define BG_GAIT_PLANES 60
int bg_env_gait_begin(bg_env* env, float* record, void* stream);
int bg_env_gait_step(bg_env* env, const uint8_t* done, int32_t settle_steps, float* record, void* stream);

/* ---- dynamics only (what north_star calls "per-step joint accelerations"): forward dynamics of N
 * independent states.  Device float arrays, env-major: root [N][13], dof_pos/dof_vel/tau [N][12],
 * base_wrench [N][6] (force, torque in base coords) or NULL; qacc out [N][18] = d/dt(lin vel world,
 * ang vel world, dof vel).  Uses the env's model, per-env parameters and terrain. */
int bg_env_forward_dynamics(bg_env* env, const float* root, const float* dof_pos, const float* dof_vel, const float* tau,
                            const float* base_wrench, float* qacc, void* stream);
/* The same call through the PACKED kernel: one env per wavefront lane, its two legs in the halves of 64-bit register pairs (v_pk_fma_f32 ...),
 * instead of one leg per lane.  Same inputs, same outputs to fp32 rounding; returns -4 when the env was created with the trunk-low gate
 * (body_gate_height > terminate_height: the non-foot body contacts need the two-kernel launch).  Replaces the same reference line
 * (envs/t1.py:451 gym.simulate, dynamics only). */
int bg_env_forward_dynamics_packed(bg_env* env, const float* root, const float* dof_pos, const float* dof_vel, const float* tau,
                            const float* base_wrench, float* qacc, void* stream);

/* ---- granular simulator calls: the Isaac Gym tensor API of envs/t1.py one call at a time (lower seam).
 * A maintainer who keeps the reference's Python task logic replaces each gym.* call by the entry point named here; the fused
 * bg_env_step above is the same physics + task logic in one launch.  The tensors are CALLER-OWNED device memory in the Isaac Gym
 * layouts and are the simulator state for these calls (no hidden copy): root [N][13] = pos, quat xyzw, lin vel, ang vel (world)
 * (t1.py:215,221-222); dof [N][12][2] = (pos, vel) (t1.py:216-218); contact [N][13][3] net contact force per body, world frame
 * (t1.py:219; only the feet carry collision geometry in this build, other rows are 0); body [N][13][13] = origin pos, quat xyzw
 * (w >= 0), lin vel of the origin, ang vel, world frame (t1.py:220).  contact / body may be NULL.  Per-env parameters, model and
 * terrain are those of the env (bg_env_set_params / bg_env_set_heightfield).  These calls do not touch the env's own task state;
 * bg_env_get_state / bg_env_set_state move state between the two. */
/* gym.acquire_actor_root_state_tensor / acquire_dof_state_tensor / acquire_net_contact_force_tensor / acquire_rigid_body_state_tensor
 * (t1.py:203-220).  Allocates the library's actuation / applied-force copies on first use. */
int bg_sim_bind_state(bg_env* env, float* root, float* dof, float* contact, float* body);
/* gym.set_dof_actuation_force_tensor (t1.py:450): tau [N][12], copied; stays in force until set again */
int bg_sim_set_actuation(bg_env* env, const float* tau, void* stream);
/* gym.apply_rigid_body_force_tensors(sim, forces, torques, LOCAL_SPACE) (t1.py:522-527): force / torque [N][13][3] in each body's own
 * frame, the force acting at the body's centre of mass; copied; either may be NULL (= zero); consumed by the next bg_sim_simulate only */
int bg_sim_apply_body_wrench_local(bg_env* env, const float* force, const float* torque, void* stream);
/* gym.simulate (t1.py:451): one sim_dt step of all envs, in place on root / dof; writes contact and body.  The refresh_* calls
 * that follow in the reference (t1.py:452-455, 460-462) have nothing left to do. */
int bg_sim_simulate(bg_env* env, void* stream);
/* gym.refresh_rigid_body_state_tensor without a step (t1.py:462 after a reset): body rows from the current root / dof tensors */
int bg_sim_refresh_body_state(bg_env* env, void* stream);
/* gym.set_actor_root_state_tensor_indexed (t1.py:341,359,504) / gym.set_dof_state_tensor_indexed (t1.py:323-325): the bound tensors
 * already are the state, so these only re-derive the body rows; env_ids (device int32 [count]) is accepted for call-site parity */
int bg_sim_write_root_state(bg_env* env, const int32_t* env_ids, int32_t count, void* stream);
int bg_sim_write_dof_state(bg_env* env, const int32_t* env_ids, int32_t count, void* stream);

/* ---- PPO math (utils/utils.py:33-52, utils/runner.py:123-180), all pointers device float unless noted */
/* GAE + returns + advantage moments.  rewards [T][N] is modified in place where time_outs is set (runner.py:135).
 * sums out [3] = (sum adv, sum adv^2, count) as float64, accumulated with atomics; caller zeroes it. */
int bg_gae(int32_t T, int32_t N, float* rewards, const uint8_t* dones, const uint8_t* time_outs, const float* values,
           const float* last_values, float gamma, float lam, float* advantages, float* returns, double* sums, void* stream);
/* Fused PPO loss forward+backward over B samples with A actions (runner.py:144-174):
 * in:  mu [B][A], logstd [A], actions [B][A], old_mu [B][A], old_logstd [A], old_logp [B], adv [B] (un-normalised),
 *      adv_stats [3] (sum, sumsq, count), values [B], returns [B]
 * out: grad_mu [B][A], grad_values [B], grad_logstd [A] float64 (atomic, caller zeroes), stats [5] float64 (atomic,
 *      caller zeroes) = sums over samples of (value error^2, surrogate, bound penalty, entropy, kl).
 * adv_stats [3] float64 = bg_gae's sums (all-reduced across ranks in data-parallel runs). */
int bg_ppo_loss(int32_t B, int32_t A, const float* mu, const float* logstd, const float* actions, const float* old_mu,
                const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, const float* values,
                const float* returns, float e_clip, float bound_coef, float entropy_coef, float* grad_mu, float* grad_values,
                double* grad_logstd, double* stats, void* stream);
/* log-prob of actions under N(mu, exp(logstd)) summed over A (runner.py:123-125) */
int bg_gaussian_logp(int32_t B, int32_t A, const float* mu, const float* logstd, const float* actions, float* logp, void* stream);
/* Fused actor inference for the rollout (utils/model.py:29-32 + dist.sample(), runner.py:109-111): 47->256->128->128->12 ELU MLP + Gaussian sample, in
 * two entry points.  bg_actor_pack copies the parameters (torch layout: w0[256][47] b0[256] w1[128][256] b1 w2[128][128] b2 w3[12][128] b3, logstd[12])
 * into `packed`, BG_ACTOR_PACKED_FLOATS floats, 16-byte aligned, in the order the sampling kernel's lanes consume them (layout: csrc/bg_ppo.hip; the
 * first layer zero-padded from 47 to 48 columns): one small launch.  bg_actor_sample reads ONLY the packed copy: obs [N][47]; out: mu [N][12] (may be
 * NULL), actions [N][12] = mu + exp(logstd) n, noise from Philox(seed, row, counter, RS_ACTOR + group of 4 actions).  A packed copy is a snapshot: it
 * does not follow later changes of the parameters; the caller packs again (the rollout does at its start, every iteration). */
#define BG_ACTOR_PACKED_FLOATS 65616
int bg_actor_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                  const float* logstd, float* packed, void* stream);
int bg_actor_sample(int32_t N, const float* obs, const float* packed, uint64_t seed, uint64_t counter, float* mu, float* actions, void* stream);
/* One Linear layer of an MLP for bg_actor_sample_mlp: W [out][in] row-major (torch layout), b [out]. */
typedef struct bg_mlp_layer_desc {
    const float* W;
    const float* b;
    int32_t in, out;
} bg_mlp_layer_desc;
/* bg_actor_sample at any supported actor architecture (utils/model.py:8-25 with configured widths + dist.sample(), runner.py:109-111), one
 * launch: layers [n_layers] = 2 to 4 hidden ELU layers (widths multiples of 128 up to 512) and the 12-wide output layer; the first layer's
 * `in` is the row stride of obs: 47 H, H = 1 .. 10 observation frames (bg_env_cfg.frame_stack).  Weight matrices after the first 16-byte aligned.  Same noise as bg_actor_sample: Philox(seed, row, counter, RS_ACTOR + group of 4 actions).
 * mu [N][12] may be NULL. */
int bg_actor_sample_mlp(int32_t N, const float* obs, int32_t n_layers, const bg_mlp_layer_desc* layers, const float* logstd, uint64_t seed,
                        uint64_t counter, float* mu, float* actions, void* stream);
/* The same launch on the rows of a perceptive actor (bg_env_cfg.actor_heights): the first layer's `in` is 47 H + scan_points, the height scan behind
 * the H observation frames, BG_ACTOR_MAX_INPUT at most (the first layer's k-chunks of 48 columns run over the frames' boundaries; columns past
 * `in` read as zeros).  scan_points = 0 is bg_actor_sample_mlp. */
int bg_actor_sample_mlp_scan(int32_t N, const float* obs, int32_t n_layers, const bg_mlp_layer_desc* layers, int32_t scan_points, const float* logstd,
                             uint64_t seed, uint64_t counter, float* mu, float* actions, void* stream);
/* Teacher-student distillation (utils/distill.py), the rollout's launch: TWO networks of bg_actor_sample_mlp's kind on the same rows.  obs [N] rows of
 * obs_stride floats = the perceptive teacher's row [47 H observations | scan_points height-scan values]; obs_stride must equal the teacher's first-layer
 * `in` (47 H + scan_points <= BG_ACTOR_MAX_INPUT) and the student's first-layer `in` must be 47 H: the student reads columns [0, 47 H) of each row and
 * samples actions [N][12] = mu_s + exp(student_logstd) n with bg_actor_sample_mlp's noise (Philox(seed, row, counter, RS_ACTOR + group of 4 actions)),
 * student_mu [N][12] may be NULL; the teacher reads all columns and writes its mean teacher_mu [N][12] only.  Width rules per network as
 * bg_actor_sample_mlp; depths and widths may differ.  The grid is split between the networks (16 rows per workgroup each), every half running the
 * stand-alone kernel's layer code: teacher_mu equals bg_actor_sample_mlp_scan's mu and student_mu / actions equal bg_actor_sample_mlp's on a
 * contiguous copy of the prefix columns, bit for bit. */
int bg_distill_act(int32_t N, const float* obs, int32_t obs_stride, int32_t n_student, const bg_mlp_layer_desc* student, int32_t n_teacher,
                   const bg_mlp_layer_desc* teacher, int32_t scan_points, const float* student_logstd, uint64_t seed, uint64_t counter, float* student_mu,
                   float* actions, float* teacher_mu, void* stream);
/* bg_distill_act for a student with a longer history than its teacher (bg_env_cfg.student_frame_stack): the same split grid and layer code, the student
 * half reading its own buffer.  teacher_obs [N] rows of teacher_stride floats = [47 H | scan_points], teacher_stride = the teacher's first-layer `in`;
 * student_obs [N] rows of student_stride floats = [47 Hs], student_stride = the student's first-layer `in` = 47 Hs, 1 <= Hs <= BG_MAX_FRAME_STACK and
 * 47 Hs >= 47 H (each violation -4, the message naming the side).  One LDS form for both halves: the wider input tile and the wider hidden layer of
 * the two decide (a student of 6 frames or more pads to 288 columns and takes the 512-wide form at any widths).  teacher_mu equals
 * bg_actor_sample_mlp_scan's mu on teacher_obs, student_mu / actions equal bg_actor_sample_mlp's on student_obs, bit for bit; bg_distill_act is this
 * call with student_obs = teacher_obs and student_stride = teacher_stride, the one case in which student_stride is not the student's `in` (which
 * must then be the teacher's 47 H). */
int bg_distill_act_hist(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride, int32_t n_student,
                        const bg_mlp_layer_desc* student, int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points,
                        const float* student_logstd, uint64_t seed, uint64_t counter, float* student_mu, float* actions, float* teacher_mu, void* stream);
/* bg_distill_act_hist with DAgger's mixing (T1.yaml distillation.teacher_action_prob): per row the teacher acts with probability beta, else the student.
 * Arguments and rules of bg_distill_act_hist (the same buffer and stride twice: bg_distill_act's case) plus beta in [0, 1] (outside it, or not finite:
 * -1, the message naming beta, before any launch) and teacher_noise.  Per row: u = entry 0 of Philox(seed, row, counter, RS_DAGGER = 29), the teacher
 * acts iff u < beta (fp32).  student_mu and teacher_mu are bg_distill_act_hist's.  actions[row]: the student acts: bg_distill_act_hist's value, mu_s +
 * exp(student_logstd) n; the teacher acts: mu_t + exp(student_logstd) n with the SAME n (Philox(seed, row, counter, RS_ACTOR + group of 4 actions)),
 * or mu_t alone with teacher_noise = 0.  One launch on the split grid: both halves evaluate u, the half that acts writes the row (disjoint rows: no
 * atomics, no second pass).  beta = 0 equals bg_distill_act_hist in all three outputs, beta = 1 gives bg_actor_sample_mlp_scan's actions of the
 * teacher under the student's logstd, bit for bit. */
int bg_distill_act_mix(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride, int32_t n_student,
                       const bg_mlp_layer_desc* student, int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points,
                       const float* student_logstd, uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise, float* student_mu, float* actions,
                       float* teacher_mu, void* stream);
/* The rollout's launch with a learned state estimator in front of the actor (T1.yaml estimator.enabled; the privileged quantities it regresses are
 * columns of the reference's privileged observation, envs/t1.py:593-602; the actor is utils/model.py:8-25 + dist.sample(), runner.py:109-111): TWO
 * networks of bg_actor_sample_mlp's kind on the same rows, one behind the other in the same workgroup.  obs [N][47 H] contiguous; est [n_est]: an MLP
 * 47 H -> hidden -> 12 (est[0].in = 47 H) whose 12 means go to est_out [N][12]; actor [n_actor]: its first layer takes 47 H + est_cols inputs
 * (1 <= est_cols <= 12; actor[0].in = est[0].in + est_cols <= BG_ACTOR_MAX_INPUT), the row [obs | est_out[:est_cols]] that the workgroup builds in LDS
 * (no round trip through memory, no copy), and it samples actions [N][12] with bg_actor_sample_mlp's noise (Philox(seed, row, counter, RS_ACTOR + group
 * of 4 actions)); mu [N][12] may be NULL.  Width rules per network as bg_actor_sample_mlp, the actor's those of scan_points = est_cols; a violation is
 * -4 or -1 with a message naming the side, before any launch.  One LDS form for both: the 256-wide form when both networks' widest hidden layer is at
 * most 256 and the actor's padded input tile at most 256 columns.  est_out equals bg_actor_sample_mlp's mu of the estimator on obs, and mu / actions
 * equal bg_actor_sample_mlp_scan(scan_points = est_cols) of the actor on a contiguous copy of [obs | est_out[:, :est_cols]], bit for bit.  Nothing is
 * written past row N. */
int bg_actor_sample_est(int32_t N, const float* obs, int32_t n_est, const bg_mlp_layer_desc* est, int32_t est_cols, int32_t n_actor,
                        const bg_mlp_layer_desc* actor, const float* logstd, uint64_t seed, uint64_t counter, float* est_out, float* mu, float* actions,
                        void* stream);
/* Random network distillation (T1.yaml rnd.enabled; rsl_rl's rnd_cfg, Burda et al. 2018): the rollout's launch behind the env step.  TWO networks of
 * bg_actor_sample_mlp's kind on the same state rows, one behind the other in the same workgroup: `target` (random, never trained) and `predictor`,
 * each an MLP K -> hidden -> 12 with K = obs_cols + priv_cols (1 <= K <= BG_ACTOR_MAX_INPUT, any K; hidden widths as bg_actor_sample_mlp).  The state
 * row is [obs row | priv row], the two blocks contiguous each ([N][obs_cols], [N][priv_cols]; priv NULL with priv_cols 0 and only then) and joined in
 * LDS, without a concatenated copy.  Per row r < N:
 *   target_out[r][0..12) = target(s);  rho = sqrt(sum_j (predictor(s)_j - target(s)_j)^2), the 12 terms added in ascending j in fp32;
 *   intrinsic[r] = dones[r] ? 0 : rho;  and, where weight != 0 and dones[r] == 0,
 *   rewards[r] = (float)((double)rewards[r] + (double)weight * reward_stats[2] * rho)      (one rounding to fp32)
 * reward_stats: device fp32 [3] = (mean, sigma, 1 / sigma) as bg_value_norm_update writes it, of which 1 / sigma alone is read; NULL = 1.  With
 * weight == 0 (of either sign) rewards is not written at all; a row with dones never is.  weight: a finite number >= 0, else -1.  Both embeddings equal
 * the mu of bg_actor_sample_mlp_scan of the network on a contiguous copy of the rows, bit for bit.  One LDS form for both networks: the 256-wide form
 * when both networks' widest hidden layer and the padded state tile (K rounded up to whole 48-column k-chunks) are at most 256 columns.  A violation
 * is -1 or -4 with a message naming the side, before any launch.  No atomics; nothing is written past row N. */
int bg_rnd_reward(int32_t N, const float* obs, int32_t obs_cols, const float* priv, int32_t priv_cols, int32_t n_target, const bg_mlp_layer_desc* target,
                  int32_t n_pred, const bg_mlp_layer_desc* predictor, const uint8_t* dones, const float* reward_stats, float weight, float* target_out,
                  float* intrinsic, float* rewards, void* stream);
/* A recurrent student (T1.yaml distillation.student_memory; rsl_rl's recurrent student of `Distillation`): a GRU cell in torch.nn.GRUCell's layout and
 * gate order r | z | n, W_ih [3 hidden][in], W_hh [3 hidden][hidden] (16-byte aligned), b_ih / b_hh [3 hidden]:
 *   gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh, r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h.
 * in = 47 (the newest single observation), hidden = 128 or 256; anything else is -4. */
typedef struct bg_gru_desc {
    const float *W_ih, *W_hh, *b_ih, *b_hh;
    int32_t in, hidden;
} bg_gru_desc;
/* bg_actor_sample_mlp with the cell in front: per row x = columns [0, 47) of obs (rows obs_stride >= 47 floats apart), h = h_in [N][hidden] (read as
 * zero where reset [N] (uint8, may be NULL) is non-zero), h' to h_out [N][hidden], and the trunk `layers` (layers[0].in = hidden, then
 * bg_actor_sample_mlp's width rules, every matrix 16-byte aligned) on h': mu [N][12] (may be NULL), actions = mu + exp(logstd) n with
 * bg_actor_sample_mlp's noise (Philox(seed, row, counter, RS_ACTOR + group of 4 actions)).  h_in == h_out is allowed: a workgroup reads its 16 rows
 * before it writes them.  Nothing is written past row N.  Violations: -1 / -4 with a message, before any launch. */
int bg_actor_sample_gru(int32_t N, const float* obs, int32_t obs_stride, const bg_gru_desc* gru, int32_t n_layers, const bg_mlp_layer_desc* layers,
                        const float* logstd, uint64_t seed, uint64_t counter, const uint8_t* reset, const float* h_in, float* h_out, float* mu,
                        float* actions, void* stream);
/* bg_distill_act_mix's split grid with the recurrent student in the student's half: the teacher's half is unchanged (teacher_mu equals
 * bg_actor_sample_mlp_scan's mean, bit for bit), the student's half is bg_actor_sample_gru's body on columns [0, 47) of the teacher's rows (student_mu,
 * h_out, and at beta = 0 actions equal bg_actor_sample_gru's, bit for bit).  beta in [0, 1] and teacher_noise: bg_distill_act_mix's rules (the same
 * RS_DAGGER draw decides which half acts; a teacher-driven row carries the student's noise draw); the memory advances on every row, whoever acts. */
int bg_distill_act_gru(int32_t N, const float* teacher_obs, int32_t teacher_stride, int32_t n_teacher, const bg_mlp_layer_desc* teacher,
                       int32_t scan_points, const bg_gru_desc* gru, int32_t n_student, const bg_mlp_layer_desc* student, const float* student_logstd,
                       uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise, const uint8_t* reset, const float* h_in, float* h_out,
                       float* student_mu, float* actions, float* teacher_mu, void* stream);
/* bg_distill_act_gru with the cell's 47 inputs from rows of the student's own: columns [0, 47) of student_obs (rows student_stride >= 47 floats apart)
 * in place of the teacher's rows (a student row that is no prefix of the teacher's: bg_env_cfg.sensor_model = 2).  The same kernel; the teacher's half
 * is untouched.  With student_obs on rows that equal the teacher's first 47 columns, every output and the state equal bg_distill_act_gru's, bit for bit. */
int bg_distill_act_gru_own(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride, int32_t n_teacher,
                           const bg_mlp_layer_desc* teacher, int32_t scan_points, const bg_gru_desc* gru, int32_t n_student, const bg_mlp_layer_desc* student,
                           const float* student_logstd, uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise, const uint8_t* reset,
                           const float* h_in, float* h_out, float* student_mu, float* actions, float* teacher_mu, void* stream);
/* The recurrence of the recurrent student's update over T steps as ONE launch each way (csrc/bg_gru.hip); H = 128 or 256, any N >= 1, T >= 1.  Envs are
 * independent: a workgroup owns 16 rows and walks the steps itself, its state tile in LDS; W_hh [3H][H] (16-byte aligned) streams from L2.
 * Forward: gi [T][N][3H] the x-side pre-activations (b_ih included), h0 [N][H] the state entering step 0 (NULL: zero), reset [T][N] (uint8, NULL: none):
 * non-zero = the state entering step t is zero.  Out: h_prev [T][N][H] the state entering each step after the reset, h [T][N][H] the new state,
 * gates [T][N][4H] = r | z | n | gh_n.  Deterministic; nothing is written past row N of any step. */
int bg_gru_sequence_forward(int32_t T, int32_t N, int32_t H, const float* gi, const float* h0, const uint8_t* reset, const float* W_hh, const float* b_hh,
                            float* h_prev, float* h, float* gates, void* stream);
/* Back-propagation through those T steps from dh_ext [T][N][H] = dL/dh[t] of whatever reads h[t]; walks t = T - 1 .. 0 with a carried dh (zero at T - 1):
 *   dh = dh_ext[t] + carry, dn = dh (1 - z), dz = dh (h_prev - n), dn_pre = dn (1 - n^2), dz_pre = dz z (1 - z), dr_pre = dn_pre gh_n r (1 - r),
 *   dgi[t] = [dr_pre | dz_pre | dn_pre], dgh[t] = [dr_pre | dz_pre | dn_pre r] (both [T][N][3H]), carry = dh z + dgh[t] W_hh, zero for a row with reset[t].
 * dh0 [N][H] (may be NULL): the carry left after step 0.  Deterministic. */
int bg_gru_sequence_backward(int32_t T, int32_t N, int32_t H, const float* dh_ext, const float* gates, const float* h_prev, const uint8_t* reset,
                             const float* W_hh, float* dgi, float* dgh, float* dh0, void* stream);
/* Several such recurrences as ONE launch each way (a PPO update with a recurrent critic beside the recurrent actor, T1.yaml algorithm.rnn_critic, where
 * both cells' recurrences would otherwise follow each other on one stream; a recurrence's time hardly depends on its number of envs).  A problem holds
 * the arguments of the single entry point by the same names; 1 to 4 problems share one H (128 or 256), each with its own T, N and pointers.  A workgroup
 * serves one problem through the single launches' own code, so every output equals theirs bit for bit, and the problems' workgroups alternate in
 * dispatch order (round r: workgroup r of every problem that has one).  Checked before any launch, with a message naming the entry point: no problem,
 * more than 4, a T or N below 1, a null pointer other than h0 / reset / dh0 (-1); a W_hh that is not 16-byte aligned (-1); an unsupported H (-4). */
typedef struct bg_gru_forward_problem {
    int32_t T, N;
    const float* gi;
    const float* h0;       /* may be NULL: zero */
    const uint8_t* reset;  /* may be NULL: none */
    const float* W_hh;
    const float* b_hh;
    float* h_prev;
    float* h;
    float* gates;
} bg_gru_forward_problem;
typedef struct bg_gru_backward_problem {
    int32_t T, N;
    const float* dh_ext;
    const float* gates;
    const float* h_prev;
    const uint8_t* reset;  /* may be NULL: none */
    const float* W_hh;
    float* dgi;
    float* dgh;
    float* dh0;            /* may be NULL: not written */
} bg_gru_backward_problem;
#define BG_GRU_GROUP_MAX 4
int bg_gru_sequence_forward_group(const bg_gru_forward_problem* problems, int32_t n_problems, int32_t H, void* stream);
int bg_gru_sequence_backward_group(const bg_gru_backward_problem* problems, int32_t n_problems, int32_t H, void* stream);
/* The cell's bias gradients of a PPO update on a recurrent actor (T1.yaml algorithm.rnn_hidden_size), without their finish: ONE launch in which
 * workgroup g sums rows [128 g, min(128 g + 128, B)) of dgi and dgh ([B][3H] each, as bg_gru_sequence_backward leaves them) down their columns and writes
 * record g of `records` ([ceil(B / 128)][6H] floats) = dgi's 3H column sums | dgh's.  Rows at or beyond B are never read, nothing is written past record
 * ceil(B / 128); fixed order, no atomics: deterministic.  The finish is the caller's bg_reduce_problem with partial = records, groups = ceil(B / 128),
 * record = n_out = 6H, out[0] = b_ih's gradient, out[1] = b_hh's, n = 3H each, in a bg_reduce_group / bg_update_tail.  B >= 1; H = 128 or 256 (else -4);
 * the three pointers 16-byte aligned (-1). */
int bg_gru_bias_partial(int32_t B, int32_t H, const float* dgi, const float* dgh, float* records, void* stream);
/* Fused global-norm clip + Adam over one flat parameter buffer (runner.py:162-165); lr is read from device memory
 * so the KL-adaptive schedule (runner.py:174-180) needs no host sync.  gnorm_scratch [1] device float64. */
int bg_adam_step(int32_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* lr_device, int32_t step,
                 float beta1, float beta2, float eps, float max_grad_norm, double* gnorm_scratch, void* stream);
/* KL-adaptive learning rate on the device (runner.py:174-180): kl_sum [1] float64 (= stats[4] of bg_ppo_loss), count = samples -> lr_device [1] updated in place */
int bg_adapt_lr(const double* kl_sum, float count, float desired_kl, float lr_min, float lr_max, float* lr_device, void* stream);
/* A second copy of one [rows][cols] row-major weight matrix of the flat parameter buffer that bg_optimizer_step keeps current while it updates the
 * parameters: transpose = 0: dst[r * ld + c] (ld >= cols: e.g. the first layer with its input columns zero-padded; the padding is not touched),
 * transpose = 1: dst[c * ld + r] (ld >= rows: the operand layout of bg_mlp_layer_backward).  offset = index of W[0][0] in params.
 * transpose = 2 / 3: dst = the bf16 planes of W / of W^T as bg_mlp_split_weights(transpose = 0 / 1) writes them (uint16_t [n_out][ld / 32][3][32],
 * 16-byte aligned, ld = k_out a multiple of 32 and >= cols / rows): what the chained split kernels read.  Elements outside the matrix (the
 * zero-padded input columns of a first layer) are not touched: write them once with bg_mlp_split_weights.  pad > 0 (kinds 2 / 3): the planes of
 * -W are kept as well, pad uint16 behind dst (bg_mlp_split_weights_pm's layout: pad = n_out * k_out * 3). */
typedef struct bg_param_mirror {
    int32_t offset, rows, cols, transpose, ld, pad;
    float* dst;
} bg_param_mirror;
/* The tail of a mini-epoch in one launch (runner.py:162-180): global-norm clip + Adam on the flat buffers (as bg_adam_step), then the KL rule on
 * lr_device (as bg_adapt_lr, with kl_sum = stats[kl_index]), and the bookkeeping of the float64 loss statistics: stats_last = stats,
 * stats_acc += stats, stats = 0 (and grad_logstd = 0) for the next mini-epoch.  grad_logstd (optional, float64 [ls_n]) is the log-std gradient as
 * the head kernels accumulate it; it is written into grads[ls_off .. ls_off + ls_n) first.  stats may be NULL (no learning-rate rule, no
 * bookkeeping).  ticket: one zero-initialised uint32 of device memory owned by the caller (the launch leaves it zero).  grads 16-byte aligned (-1
 * otherwise).  mirrors (optional, up to 16): see bg_param_mirror.  Deterministic (no float atomics). */
int bg_optimizer_step(int32_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* lr_device, int32_t step, float beta1, float beta2,
                      float eps, float max_grad_norm, double* grad_logstd, int32_t ls_off, int32_t ls_n, double* stats, double* stats_acc,
                      double* stats_last, int32_t n_stats, int32_t kl_index, float kl_count, float desired_kl, float lr_min, float lr_max,
                      uint32_t* ticket, const bg_param_mirror* mirrors, int32_t n_mirrors, void* stream);

/* MLP backward helper for the ELU layers of utils/model.py:9-26: grad [B][C] <- grad * elu'(.) in place, expressed through the layer OUTPUT
 * act [B][C] (1 if act > 0 else act + 1; act == NULL: identity), and colsum [C] = column sums of the result (= bias gradient).
 * scratch: ceil(B/128) * C floats.  No alignment is asked of any buffer; with act, C a power of two from 4 to 256 and grad, act and scratch all 16-byte aligned a
 * wider form runs that adds the same terms of a column in another fixed order (colsum's bits then depend on the alignment, on nothing else).
 * Deterministic (no atomics). */
int bg_elu_backward_colsum(int32_t B, int32_t C, float* grad, const float* act, float* colsum, float* scratch, void* stream);

/* Fused MLP layer forward: Y [M][N] = act(X [M][K] . W[N][K]^T + bias[N]) in fp32 MFMA with bias + ELU in the GEMM epilogue
 * (utils/model.py:9-26 Linear + ELU).  Supported: K in {64, 128, 256, 512}, N a multiple of 128 up to 1024; other shapes return -4 (caller uses the
 * library GEMM).  X, W, bias and Y 16-byte aligned (-1 otherwise).  Exactly the M rows of Y are written; rows of X at or beyond M are never read. */
int bg_mlp_layer_forward(int32_t M, int32_t K, int32_t N, const float* X, const float* W, const float* bias, float* Y, int32_t elu, void* stream);
/* The three hidden Linear + ELU layers of one network (utils/model.py:9-26, forward of runner.py:132,147) in ONE launch: Y1 = elu(X W1^T + b1) [M][N1],
 * Y2 = elu(Y1 W2^T + b2) [M][N2], Y3 = elu(Y2 W3^T + b3) [M][N3], every activation stored for the backward pass; between the layers the
 * activations stay in registers (bg_mlp_chain.hip).  X [M][K0] with K0 = 64 (zero-padded input columns), W row-major [out][in] as torch's Linear.
 * Supported widths (N1, N2, N3): (256, 128, 128) and (256, 256, 128), the reference's actor and critic.  Y1 / Y2 / Y3 must hold
 * ceil(M / 128) * 128 rows (rows >= M of the last slab are written with unspecified values).  Bit-identical to three bg_mlp_layer_forward
 * launches.  X, W1 .. W3, b1 .. b3, Y1 .. Y3 and v_w 16-byte aligned (-1 otherwise; v_b and v_out need no alignment).  -4: unsupported widths. */
typedef struct bg_mlp_chain {
    int32_t M, K0, N1, N2, N3;
    int32_t workgroups;  /* 0: one workgroup per 128-row slab; > 0: that many workgroups walk the slabs (each fills a CU: two launches side by side then
                          * share the chip by CUs -- see bg_mlp_chain.hip).  Same outputs either way. */
    const float *X, *W1, *b1, *W2, *b2, *W3, *b3;
    float *Y1, *Y2, *Y3;
    /* optional scalar output layer on Y3 (the critic's value head, utils/model.py:21): v_out[row] = v_w . Y3[row] + v_b[0], taken from the registers that
     * hold Y3 (v_w [N3], v_b [1]; v_out [M]); all three NULL: none.  Another summation order than bg_critic_head_forward (same values to fp32 rounding). */
    const float *v_w, *v_b;
    float* v_out;
} bg_mlp_chain;
int bg_mlp_chain_forward(int32_t M, int32_t K0, int32_t N1, int32_t N2, int32_t N3, const float* X, const float* W1, const float* b1, const float* W2,
                         const float* b2, const float* W3, const float* b3, float* Y1, float* Y2, float* Y3, void* stream);
/* 1 to 4 networks in one launch; the 128-row slabs of nets[0] are dispatched first, those of the next network fill the machine as they retire. */
int bg_mlp_chain_forward_group(const bg_mlp_chain* nets, int32_t count, void* stream);

/* Fused MLP layer backward through one Linear and the ELU below it:  Gout [M][N] = (G [M][K] . Wt[N][K]^T) * elu'(act_below [M][N]) and
 * bias_grad_below [N] = column sums of Gout.  G = dL/dz of the upper layer (K = its width), Wt = that layer's weight TRANSPOSED to [N][K]
 * (N = width of the layer below), act_below = the lower layer's output activations.  scratch: ceil(M/128) * N floats.
 * Replaces torch.mm(G, W) + elu_backward + the bias-gradient reduction.  K in {128, 256, 512}, N a multiple of 128 up to 1024; otherwise -4.
 * G, Wt, act_below and Gout 16-byte aligned (-1 otherwise).  Exactly the M rows of Gout are written; rows of G / act_below at or beyond M are never read. */
int bg_mlp_layer_backward(int32_t M, int32_t K, int32_t N, const float* G, const float* Wt, const float* act_below, float* Gout,
                          float* bias_grad_below, float* scratch, void* stream);

/* Split form of the two layer kernels above (opt-in; same inputs, outputs and epilogues): the fp32 x fp32 products run on the bf16 matrix
 * pipe.  Every fp32 operand is EXACTLY the sum of three bf16 numbers (hi / mid / lo: 8 + 8 + 8 significant bits) and a bf16 x bf16 product
 * is exact in the fp32 accumulator, so terms = 9 (all cross terms) accumulates the exact products x * w in fp32 -- no precision is given up
 * against the fp32 MFMA form; terms = 6 drops mid*lo, lo*mid, lo*lo (<= 2^-23 of each product).  The weights come pre-split:
 * bg_mlp_split_weights writes planes[n_out][k_out / 32][3][32] bf16 from W [src_rows][ldw] (transpose != 0: element (n, k) = W[k][n]);
 * elements outside the source are zero (the zero-padded first layers), k_out a multiple of 32, 6 bytes per element.
 * Same N limits and error codes as bg_mlp_layer_forward / _backward; K in {64, 128, 256} forward, {128, 256} backward (K = 512 runs in the fp32
 * form only).  planes 16-byte aligned, as the other matrix pointers of the two layer kernels. */
int bg_mlp_split_weights(int32_t n_out, int32_t k_out, const float* W, int32_t ldw, int32_t src_rows, int32_t src_cols, int32_t transpose,
                         uint16_t* planes, void* stream);
/* bg_mlp_split_weights, and behind its planes (n_out * k_out * 3 uint16 further) the planes of -W: what the chained split kernels read with
 * `alternate` set (planes must hold 2 * n_out * k_out * 3 uint16). */
int bg_mlp_split_weights_pm(int32_t n_out, int32_t k_out, const float* W, int32_t ldw, int32_t src_rows, int32_t src_cols, int32_t transpose,
                            uint16_t* planes, void* stream);
int bg_mlp_layer_forward_split(int32_t M, int32_t K, int32_t N, const float* X, const uint16_t* planes, const float* bias, float* Y, int32_t elu,
                               int32_t terms, void* stream);
int bg_mlp_layer_backward_split(int32_t M, int32_t K, int32_t N, const float* G, const uint16_t* planes_t, const float* act_below, float* Gout,
                                float* bias_grad_below, float* scratch, int32_t terms, void* stream);

/* bg_mlp_chain_forward_group on the bf16 matrix pipe with fp32 semantics (bg_mlp_chain_split.hip; reference utils/model.py:9-26 under
 * utils/runner.py:132,147): the same three Linear + ELU layers per network in one launch, activations handed on in registers, every fp32 x fp32 product
 * formed exactly from the 9 cross products of the operands' three bf16 planes (see bg_mlp_layer_forward_split; terms = 9 only).  P1 / P2 / P3: the
 * layers' weight planes as bg_mlp_split_weights writes them (transpose = 0; P1 with k_out = K0 = 64, the zero-padded input width).  Same shapes, slab
 * padding of Y1 / Y2 / Y3, `workgroups` and value head as bg_mlp_chain.  Not bit-identical to the fp32-MFMA chain (another summation order; the bias is
 * the accumulators' initial value): both are exact-product fp32 sums.  1 to 4 networks per launch (each on its own `workgroups` persistent
 * workgroups inside one grid: how the update shares the chip between the critic and the actor); which workgroup walks which slab changes no bit of
 * any output (tests/test_gpu_mlp_chain_split.py).  X, P1 .. P3, b1 .. b3, Y1 .. Y3 and v_w 16-byte aligned (-1 otherwise). */
typedef struct bg_mlp_chain_split {
    int32_t M, K0, N1, N2, N3;
    int32_t workgroups;
    /* alternate != 0: odd slabs accumulate the NEGATED sums (the planes of -W: P1 / P2 / P3 then hold both sets, bg_mlp_split_weights_pm) and the
     * sign is put back where a tile is finished.  The bf16 MFMA's accumulator does not round to nearest: every accumulated element carries a small
     * bias of one sign (measured: -0.05 of the rms error), which adds up in everything summed over rows downstream (bias and weight gradients);
     * alternating the sign of the accumulation slab by slab makes the bias cancel.  Same products, same exactness.
     * slab0 >= 0: the place in its batch of the launch's first 128-row slab (X / Y1 / Y2 / Y3 / v_out point at row 128 * slab0 of a larger batch);
     * slab slab0 + s of the batch is odd or even, not slab s of the launch, so a piece leaves the bits the launch on the whole batch leaves.
     * A launch on a whole batch passes 0. */
    int32_t alternate, slab0;
    const float* X;
    const uint16_t *P1, *P2, *P3;
    const float *b1, *b2, *b3;
    float *Y1, *Y2, *Y3;
    const float *v_w, *v_b;
    float* v_out;
} bg_mlp_chain_split;
int bg_mlp_chain_forward_split(const bg_mlp_chain_split* nets, int32_t count, void* stream);

/* Weight gradient of one Linear layer over the batch (the dW part of `loss.backward()`, utils/runner.py:163, for model.py:9-26's layers):
 * dW [C_out][C_in_real] = G [M][C_out]^T . A [M][C_in][:, :C_in_real], fp32 MFMA, the sum over the M rows split over `slices` x 4 waves
 * inside the launch and finished in a fixed order (deterministic, no atomics).  G = dL/dz of the layer, A = its input activations with
 * the feature dimension C_in possibly zero-padded (the first layers: 47 / 61 -> 64); only the first C_in_real columns are written, with
 * row stride C_in_real, so dW can be the parameter's .grad view in the flat gradient buffer.
 * C_out a multiple of 128, C_in 64 or a multiple of 128, M even, slices a multiple of 8 with slices * 8 <= M;
 * scratch: slices * C_out * C_in floats.  G, A and scratch 16-byte aligned, dW too when C_in_real == C_in (a narrower dW is written float by float and
 * needs no alignment).  Otherwise -4 / -1. */
int bg_mlp_weight_grad(int32_t M, int32_t C_out, int32_t C_in, int32_t C_in_real, const float* G, const float* A, float* dW, float* scratch,
                       int32_t slices, void* stream);

/* The weight gradients of several layers in ONE launch pair (the dW part of `loss.backward()` for all hidden layers of both networks, after both
 * backward chains): same arithmetic and argument meaning per layer as bg_mlp_weight_grad; `slices` of a layer may be any value in [1, M/8] -- size
 * them so that every workgroup of the launch does the same amount of work (booster_gym_amd/utils/model.py:plan_wgrad_slices).  One workgroup per
 * (group of tiles_per_workgroup tiles, slice).  count <= 8. */
typedef struct {
    const float* G;      /* [M][C_out] dL/dz of the layer */
    const float* A;      /* [M][C_in] its input activations (feature dimension possibly zero-padded) */
    float* dW;           /* [C_out][C_in_real] */
    float* scratch;      /* slices * C_out * C_in floats */
    int32_t M, C_out, C_in, C_in_real, slices;
    int32_t tiles_per_workgroup; /* 1 (default for 0), 2 or 4, dividing the layer's count of 128-wide output tiles: the 4 waves of a workgroup cover
                                  * this many tiles x 4 / this many sub-ranges of the slice's rows; waves on the same rows share the fetched rows */
} bg_wgrad_problem;
int bg_mlp_weight_grad_group(const bg_wgrad_problem* problems, int32_t count, void* stream);
/* bg_mlp_weight_grad_group without its finishing launch: the per-slice partial tiles stay in the problems' scratch, to be summed by bg_update_tail. */
int bg_mlp_weight_grad_group_partial(const bg_wgrad_problem* problems, int32_t count, void* stream);
/* Split form of the grouped launch (the training loop's default since round 6, terms = 9; reference utils/runner.py:163): the same sums with every fp32
 * operand split exactly into three bf16 numbers on the bf16 matrix pipe, terms = 9 (every product exact) or 6.  The sub-ranges of the batch take turns
 * accumulating the NEGATED sums (the bf16 MFMA's accumulator truncates; the offsets then cancel in the sum over the batch): measured error against
 * float64 0.84-0.89 of bg_mlp_weight_grad_group's.  The waves of a workgroup that work on the same rows share them through LDS, so here
 * tiles_per_workgroup must equal the layer's tile count (1, 2 or 4).  Shapes: 256 x 256, 128 x 256, 128 x 128, 256 x 64 (C_out x C_in padded), M a
 * multiple of 32; anything else returns -4 and the caller uses bg_mlp_weight_grad_group.  Same scratch layout and fixed-order finish. */
int bg_mlp_weight_grad_group_split(const bg_wgrad_problem* problems, int32_t count, int32_t terms, void* stream);
/* ... without its finish, for bg_update_tail (as bg_mlp_weight_grad_group_partial: the same scratch layout, the same finish). */
int bg_mlp_weight_grad_group_split_partial(const bg_wgrad_problem* problems, int32_t count, int32_t terms, void* stream);

/* ---- output ("head") layers fused with the loss: the 128 -> 12 / 128 -> 1 Linear layers of utils/model.py:13,21 together with
 * runner.py:145-174.  h [rows][128] = activations of the last hidden (ELU) layer, 16-byte aligned.  One launch reads h once instead of
 * the seven library GEMM / elementwise passes these skinny layers otherwise take per network and mini-epoch.
 * scratch: BG_HEAD_SCRATCH_FLOATS floats of device memory per concurrent call, 16-byte aligned (per-workgroup partial sums, added in a fixed order:
 * up to 768 records of 12 * 128 + 128 + 16 floats and, behind them, up to 18 float64 statistics per workgroup; bg_head.hip asserts that they fit). */
#define BG_HEAD_SCRATCH_FLOATS (768 * 1720)
/* critic.6 forward: values [rows] = h w + b   (w [128], 16-byte aligned as h is (-1 otherwise); b [1]) */
int bg_critic_head_forward(int32_t rows, const float* h, const float* w, const float* b, float* values, void* stream);
/* bg_critic_head_forward on all (T + 1) N rows of h (time-major: row t N + e), then bg_gae on the result, in ONE launch (utils/runner.py:132-141: values,
 * last values, timeout bootstrap, discount_values, returns): values_all [(T + 1) N] (the last N = last_values), advantages / returns [T][N], rewards
 * overwritten at time-outs as bg_gae does, sums float64 [3] WRITTEN (sum, sum of squares, count; fixed order: deterministic).  scratch: float64
 * [3 * ceil(N / 16) + 1], its last element zero-initialised once by the caller (the launch leaves it zero).  Values bit-identical to
 * bg_critic_head_forward, advantages to bg_gae.  h == NULL: values_all is an INPUT (e.g. written by bg_mlp_chain_forward's value head) and only the
 * GAE half runs (w, b unused).  With h: h and w 16-byte aligned (-1 otherwise), in bg_critic_values_gae_norm as well.  -4: T > 32. */
int bg_critic_values_gae(int32_t T, int32_t N, const float* h, const float* w, const float* b, float* rewards, const uint8_t* dones,
                         const uint8_t* time_outs, float gamma, float lam, float* values_all, float* advantages, float* returns, double* sums,
                         double* scratch, void* stream);
/* ---- value normalisation (algorithm.normalize_value): the critic's output is u, its value v = fmaf(sigma, u, m); value_stats = device fp32
 * [3] = (m, sigma, 1 / sigma), sigma = sqrt(var) + eps.
 * bg_critic_values_gae under it: values_all keeps u (h == NULL: reads it); the time-out bootstrap written into rewards, the GAE scan, advantages and
 * sums[0..2] run on v, bit-identical to bg_value_denormalize followed by bg_critic_values_gae; returns receives (R - m) * (1 / sigma) with
 * R = v + advantage, subtract and multiply each rounded (bg_obs_normalize's rule).  sums float64 [6] WRITTEN: the three above, then sum R, sum R^2 and
 * the count of the un-normalised returns.  scratch: float64 [6 * ceil(N / 16) + 1], its last element zero-initialised once.  -4: T > 32. */
int bg_critic_values_gae_norm(int32_t T, int32_t N, const float* h, const float* w, const float* b, float* rewards, const uint8_t* dones,
                              const uint8_t* time_outs, float gamma, float lam, float* values_all, float* advantages, float* returns,
                              const float* value_stats, double* sums, double* scratch, void* stream);
/* values[i] = fmaf(sigma, values[i], m) in place, i < rows: one rounding per value */
int bg_value_denormalize(int32_t rows, float* values, const float* value_stats, void* stream);
/* Chan et al.'s merge of state float64 [3] = (mean, population variance, count) with the batch of sums[3..5] = (sum, sum of squares, count), the
 * layout bg_critic_values_gae_norm writes, in float64; then value_stats = ((float)mean, (float)sigma, (float)(1 / sigma)), sigma = sqrt(var) + eps.
 * A count of zero leaves state and value_stats as they are.  One wave. */
int bg_value_norm_update(const double* sums, double* state, float* value_stats, double eps, void* stream);
/* actor.6 forward (mode 0: mu_out [B][12] = h W^T + b, nothing else is touched) or forward + PPO actor loss + backward (mode 1), with the
 * argument meaning of bg_ppo_loss: out g_hidden [B][128] = dL/dz of the last hidden layer, grad_W [12][128], grad_b [12],
 * grad_b_hidden [128] (bias gradient of the last hidden layer = column sums of g_hidden), grad_logstd [12] float64 and
 * stats[1..4] float64 (surrogate, bound penalty, entropy, kl sums; atomic, caller zeroes; stats[0] is left to the critic head).
 * mu_out may be NULL in mode 1. */
int bg_actor_head(int32_t B, int32_t mode, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                  const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip,
                  float bound_coef, float entropy_coef, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden,
                  double* grad_logstd, double* stats, float* scratch, void* stream);
/* critic.6 backward of the value loss mean((v - ret)^2) (runner.py:148): g_hidden [B][128], grad_w [128], grad_b [1], grad_b_hidden [128],
 * stats[0] += sum of squared value errors (float64, atomic) */
int bg_critic_head_backward(int32_t B, const float* h, const float* w, const float* values, const float* returns, float* g_hidden, float* grad_w,
                            float* grad_b, float* grad_b_hidden, double* stats, float* scratch, void* stream);
/* Behaviour-cloning head of the distillation's student: mu = h W^T + b (W [12][128], b [12]; bg_actor_head's sums: the same bits as its mode 0), the
 * loss L = 1 / (12 B) sum (mu - target)^2 against target [B][12] (the teacher's means) and its backward: g_hidden [B][128] = dL/dz of the last hidden
 * layer (ELU derivative from h applied), grad_W [12][128], grad_b [12], grad_b_hidden [128], stats[0] += the sum of squared errors (float64, one
 * atomic; the caller zeroes).  mu_out [B][12] may be NULL.  Per-workgroup records in scratch, added in a fixed order: deterministic. */
int bg_distill_head(int32_t B, const float* h, const float* W, const float* bias, const float* target, float* mu_out, float* g_hidden, float* grad_W,
                    float* grad_b, float* grad_b_hidden, double* stats, float* scratch, void* stream);

/* Mirror-symmetry loss (algorithm.symmetry_loss): the actor's batch is 2B rows, rows [B, 2B) of h / g_hidden / mu_out the mirror images of rows [0, B)
 * (their observations M_o x, written by bg_mirror_rows).  bg_actor_head mode 1 on the original rows plus, with d_r = mu(M_o x_r) - M_a mu(x_r), the term
 * sym_coef / (B 12) sum_r |d_r|^2, differentiated through both means: g_hidden [2B][128], grad_W / grad_b / grad_b_hidden over all 2B rows,
 * grad_logstd as bg_actor_head, stats[1..4] as bg_actor_head and stats[5] = sum_r |d_r|^2 (float64).  M_a: act_src / act_sign (host arrays of 12),
 * (M_a v)[a] = act_sign[a] v[act_src[a]], a symmetric involution (act_src[act_src[a]] = a, act_sign[act_src[a]] = act_sign[a]; -1 otherwise).
 * Fixed-order sums as bg_actor_head; mu_out [2B][12] may be NULL. */
int bg_actor_head_sym(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions, const float* old_mu,
                      const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip, float bound_coef,
                      float entropy_coef, float sym_coef, const int32_t* act_src, const float* act_sign, float* mu_out, float* g_hidden, float* grad_W,
                      float* grad_b, float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, void* stream);
/* y [rows][cols] = the rows of x [rows][cols] mirrored: y[r][c] = sign[c] x[r][src[c]] (src[c] = -1: 0), cols <= 512, src / sign host arrays of cols,
 * sign +-1; x and y must not overlap.  Exact. */
int bg_mirror_rows(int32_t rows, int32_t cols, const int32_t* src, const float* sign, const float* x, float* y, void* stream);
/* Partner rows of the action-smoothness loss (algorithm.smoothness_loss): the second source of rows [B, 2B) of bg_actor_head_sym's batch, which then
 * runs with the identity action map (act_src = 0..11, act_sign = +1: d_r = mu(x'_r) - mu(x_r)).  x [T][N][cols] are the actor's input rows of T steps
 * of N envs, x_last [N][cols] those of the step after the last, dones / time_outs [T][N] bytes (0 / not 0).  For row r = t N + e:
 *   y[r] = x[r] + u_r (x+[r] - x[r]),  x+[r] = x[r + N] (t < T - 1) or x_last[e] (t = T - 1);
 *   dones[r] or time_outs[r] set (a reset or a command resample: where GAE cuts): y[r] = x[r], a bit-exact copy;
 *   mode BG_PARTNER_NEXT: u_r = 1, y[r] a bit-exact copy of x+[r]; seed / update / epoch are not read;
 *   mode BG_PARTNER_INTERPOLATE: u_r = (o >> 8) 2^-24 in [0, 1), o = word 0 of Philox4x32-10 on the key (seed) and the counter (r, update, 30, epoch):
 *   one draw per row, y[r][c] = fma(u_r, x+[r][c] - x[r][c], x[r][c]) in fp32.
 * cols a multiple of 4 and <= 512; x, x_last and y 16-byte aligned; y overlaps neither x nor x_last; T N < 2^31 (-1 with a message otherwise, before any
 * launch).  Deterministic, no atomics; every element of y's T N rows is written, nothing past them. */
#define BG_PARTNER_NEXT 0
#define BG_PARTNER_INTERPOLATE 1
int bg_partner_rows(int32_t T, int32_t N, int32_t cols, const float* x, const float* x_last, const uint8_t* dones, const uint8_t* time_outs, int32_t mode,
                    uint64_t seed, uint32_t update, uint32_t epoch, float* y, void* stream);
/* Mirror-symmetry loss on the distillation's student (T1.yaml distillation.symmetric_coef): bg_distill_head on a batch of 2B rows laid out as for
 * bg_actor_head_sym (h / g_hidden / mu_out [2B] rows, rows [B, 2B) the mirror images of rows [0, B); target [B][12]).  L = 1 / (12 B) sum_r |mu_r -
 * target_r|^2 over the original rows + sym_coef / (12 B) sum_r |d_r|^2, d_r = mu(M_o x_r) - M_a mu(x_r), differentiated through both means: with s = 2
 * sym_coef / (12 B), dL/dmu of a mirrored row is s d and of an original row 2 (mu - target) / (12 B) - s M_a d.  g_hidden [2B][128], grad_W / grad_b /
 * grad_b_hidden over all 2B rows, stats[0] += the sum of squared errors, stats[1] += sum_r |d_r|^2 (float64; the caller zeroes).  sym_coef finite and
 * >= 0, M_a as for bg_actor_head_sym (-1 otherwise).  mu_out [2B][12] may be NULL; its rows [0, B) are bg_distill_head's bits.  Fixed-order sums:
 * deterministic; nothing is written past row 2B. */
int bg_distill_head_sym(int32_t B, const float* h, const float* W, const float* bias, const float* target, float sym_coef, const int32_t* act_src,
                        const float* act_sign, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden, double* stats, float* scratch,
                        void* stream);

/* ---- deferred fixed-order reductions.  The head kernels and the backward layer kernel leave per-workgroup partial sums that a small second
 * kernel adds up (head: output-layer weight / bias gradients, last hidden layer's bias gradient, float64 loss statistics; backward layer: the
 * bias gradient of the layer below).  None of these sums is needed before the optimiser step (utils/runner.py:162-165), so instead of one small
 * launch in the middle of each network's chain (40 + 80 launches per PPO iteration that wait for workgroup slots between the GEMMs) the
 * `_partial` forms below launch the main kernel only and fill a descriptor; bg_reduce_group then runs all descriptors of a mini-epoch in ONE
 * launch, e.g. on a second stream beside the weight-gradient launch.  Same sums, same fixed order as the immediate forms for the heads; the
 * column sums of the backward layer are added in a different (still fixed) order than bg_mlp_layer_backward's own finish. */
typedef struct {
    const float* partial;           /* [groups][record] floats */
    int32_t groups, record, n_out;  /* out[i] = sum over g of partial[g * record + i], i < n_out */
    float* out[3]; int32_t n[3];    /* element i < n[0] goes to out[0][i], the next n[1] to out[1], the rest to out[2] (unused: NULL / 0) */
    /* optional float64 statistics, statistic-major [n_stat][groups] at (partial + stat_base): statistic k < n_ls is added (+ entropy_coef) to
     * grad_logstd[k], the others to stats[k - n_ls]; bit k of stat_skip skips statistic k */
    uint64_t stat_base; int32_t n_stat, n_ls; uint32_t stat_skip; double entropy_coef; double* grad_logstd; double* stats;
} bg_reduce_problem;
int bg_reduce_group(const bg_reduce_problem* problems, int32_t count, void* stream); /* count <= 8 */
/* bg_actor_head_sym without its finishing launch (as bg_actor_head_partial). */
int bg_actor_head_sym_partial(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions, const float* old_mu,
                              const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip, float bound_coef,
                              float entropy_coef, float sym_coef, const int32_t* act_src, const float* act_sign, float* mu_out, float* g_hidden, float* grad_W,
                              float* grad_b, float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, bg_reduce_problem* finish, void* stream);
/* The backward-data chain of one network in ONE launch on the bf16 matrix pipe with fp32 semantics (bg_mlp_chain_split_bwd.hip; the dX part of
 * `loss.backward()`, utils/runner.py:163, through utils/model.py:9-26's hidden layers):  G2 [M][N2] = (G3 [M][N3] . W3 [N3][N2]) * elu'(A2),
 * G1 [M][N1] = (G2 . W2 [N2][N1]) * elu'(A1), and the column sums of G2 / G1 (the bias gradients of layers 2 / 1: bg_mlp_layer_backward twice).
 * PT3 / PT2: the planes of W3^T / W2^T as bg_mlp_split_weights(transpose = 1) writes them ([N2][N3 / 32][3][32], [N1][N2 / 32][3][32]); A2 / A1: the
 * layers' stored outputs, holding ceil(M / 128) * 128 rows of finite values as bg_mlp_chain_forward_split leaves them (whole 128-byte rows of a
 * slab are copied; rows >= M do not enter the results).  G2 / G1 must hold ceil(M / 128) * 128 rows (rows >= M are written with zeros).  Every wave
 * leaves one record of column sums per slab in colsum_partial ([ceil(M / 128) * 4][N2 + N1] floats); `finishes[k]` receives the descriptor of the
 * fixed-order reduction that produces bias_grad2 [N2] and bias_grad1 [N1] when handed to bg_reduce_group / bg_update_tail.  Widths (N1, N2, N3):
 * (256, 128, 128), (256, 256, 128).  1 to 4 networks per launch; `workgroups` as in bg_mlp_chain_split: which workgroup walks which slab changes no
 * bit of any output.  G3, PT3, PT2, A2, A1, G2 and G1 16-byte aligned (-1 otherwise); colsum_partial and the bias gradients need no alignment. */
typedef struct bg_mlp_chain_split_bwd {
    int32_t M, N1, N2, N3;
    int32_t workgroups, alternate;   /* alternate: as in bg_mlp_chain_split; PT3 / PT2 then hold the planes of W^T and of -W^T */
    const float* G3;
    const uint16_t *PT3, *PT2;
    const float *A2, *A1;
    float *G2, *G1;
    float* colsum_partial;
    float *bias_grad2, *bias_grad1;
} bg_mlp_chain_split_bwd;
int bg_mlp_chain_backward_split(const bg_mlp_chain_split_bwd* nets, int32_t count, bg_reduce_problem* finishes, void* stream);

/* The tail of a mini-epoch behind bg_mlp_weight_grad_group_partial (runner.py:162-180: the last sums of loss.backward(), clip_grad_norm_,
 * optimizer.step(), the KL rule) as two launches: (1) the weight gradients' fixed-order finish over their slices (wgrad: the problems handed to the
 * _partial launch; 0: none) and the deferred reductions (reduce: as bg_reduce_group; 0: none), every block also leaving the sum of the squares of the
 * gradient values it wrote; (2) everything bg_optimizer_step does (same arguments), with the global norm taken from those sums instead of a pass over
 * the whole gradient per workgroup.  REQUIRES that the two lists together produce every element of grads except the log-std slice (true for the
 * reference's networks: hidden-layer weights from the weight gradients, all biases and the output layers from the reductions); elements they do not
 * write must be zero.  Gradients: the same bits as the separate launches; the norm is summed in another (fixed) order.  sync: uint32 [1],
 * zero-initialised once by the caller (the launch leaves it zero); norm_scratch: float64 [BG_TAIL_MAX_BLOCKS], one slot per block of launch (1): a
 * call whose two lists need more blocks is refused (-4). */
#define BG_TAIL_MAX_BLOCKS 8192
int bg_update_tail(const bg_wgrad_problem* wgrad, int32_t n_wgrad, const bg_reduce_problem* reduce, int32_t n_reduce, int32_t n, float* params, float* grads,
                   float* exp_avg, float* exp_avg_sq, float* lr_device, int32_t step, float beta1, float beta2, float eps, float max_grad_norm,
                   double* grad_logstd, int32_t ls_off, int32_t ls_n, double* stats, double* stats_acc, double* stats_last, int32_t n_stats, int32_t kl_index,
                   float kl_count, float desired_kl, float lr_min, float lr_max, uint32_t* sync, double* norm_scratch, const bg_param_mirror* mirrors,
                   int32_t n_mirrors, void* stream);
/* Launch (1) of bg_update_tail alone, for the ranks of a multi-GPU job: the gradient's last sums, THEN the all-reduce over the ranks, THEN
 * bg_optimizer_step, which takes the norm of the averaged gradient itself (the reference clips what `loss.backward()` left on its one process,
 * runner.py:162-165; under data parallelism that is the mean over the ranks).  norm_scratch: float64 [BG_TAIL_MAX_BLOCKS] (written, not used by the caller). */
int bg_update_tail_sums(const bg_wgrad_problem* wgrad, int32_t n_wgrad, const bg_reduce_problem* reduce, int32_t n_reduce, double* norm_scratch, void* stream);
/* bg_actor_head mode 1 / bg_critic_head_backward / bg_mlp_layer_backward without their finishing launch: same arguments, plus the descriptor
 * of the reduction that produces grad_W, grad_b, grad_b_hidden, grad_logstd, stats / bias_grad_below when handed to bg_reduce_group. */
int bg_actor_head_partial(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                          const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip,
                          float bound_coef, float entropy_coef, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden,
                          double* grad_logstd, double* stats, float* scratch, bg_reduce_problem* finish, void* stream);
int bg_critic_head_backward_partial(int32_t B, const float* h, const float* w, const float* values, const float* returns, float* g_hidden,
                                    float* grad_w, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish,
                                    void* stream);
int bg_mlp_layer_backward_partial(int32_t M, int32_t K, int32_t N, const float* G, const float* Wt, const float* act_below, float* Gout,
                                  float* bias_grad_below, float* scratch, bg_reduce_problem* finish, void* stream);
/* bg_distill_head without its finishing launch (as bg_actor_head_partial). */
int bg_distill_head_partial(int32_t B, const float* h, const float* W, const float* bias, const float* target, float* mu_out, float* g_hidden, float* grad_W,
                            float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish, void* stream);
/* bg_distill_head_sym without its finishing launch (as bg_actor_head_partial). */
int bg_distill_head_sym_partial(int32_t B, const float* h, const float* W, const float* bias, const float* target, float sym_coef, const int32_t* act_src,
                                const float* act_sign, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden, double* stats,
                                float* scratch, bg_reduce_problem* finish, void* stream);

/* ---- empirical observation normalisation (algorithm.empirical_normalization; bg_obs_norm.hip).  Two launches of their own beside the hot path:
 * nothing of them runs when the key is false.
 *
 * bg_obs_moments: sum[c] = sum over r of x[r][c] and sumsq[c] = sum over r of x[r][c]^2 in float64 for the row-major fp32 matrix x [rows][cols_a +
 * cols_b] given as two column blocks with their own row strides in floats (a: columns [0, cols_a), 1 to 512; b: the cols_b columns behind them,
 * 0 to 201, b may be NULL when cols_b is 0): the observation and the privileged block of an experience buffer, without a concatenated copy.
 * Fixed summation order, no floating-point atomics: every workgroup leaves one record [2][cols_a + cols_b] in `scratch` (float64, at least
 * BG_OBS_MOMENTS_MAX_GROUPS * 2 * (cols_a + cols_b) values) and a second small launch adds the records in a fixed order; the grid depends on `rows`
 * alone, so the same input gives the same bits on every device.  sum / sumsq: float64 [cols_a + cols_b], overwritten. */
#define BG_OBS_MOMENTS_MAX_GROUPS 1024
int bg_obs_moments(int32_t rows, const float* a, int32_t cols_a, int32_t stride_a, const float* b, int32_t cols_b, int32_t stride_b, double* sum,
                   double* sumsq, double* scratch, void* stream);
/* dst[r][c] = (src[r][c] - mean[col0 + c]) * inv_std[col0 + c] for c < cols and 0 for cols <= c < dst_cols, r < rows: the fp32 subtract rounded,
 * then the fp32 multiply rounded (never contracted), so every call gives the same bits for the same row.  src_stride / dst_stride: row strides in
 * floats (cols <= src_stride, cols <= dst_cols <= dst_stride); dst_cols - cols = the zero padding of a network input behind the block (dst_cols at
 * most 512); col0 + cols at most 713.  src is not written; src and dst must not overlap. */
int bg_obs_normalize(int32_t rows, int32_t cols, const float* src, int32_t src_stride, float* dst, int32_t dst_cols, int32_t dst_stride,
                     const float* mean, const float* inv_std, int32_t col0, void* stream);

/* ---- shuffled mini-batches of the PPO update (runner.num_mini_batches > 1; bg_minibatch.hip).  Two launches of their own per mini-epoch: nothing of
 * them runs when the key is absent or 1.
 *
 * bg_perm_fill: perm[i] = pi(i), i < n, for the permutation pi of [0, n) that the key (seed, update, epoch) names: a balanced Feistel network on
 * ceil(log2 n) bits (rounded up to an even number) whose round functions are philox4x32_10 draws, with cycle walking for images at or beyond n
 * (csrc/bg_perm.h, which also compiles for the host).  Evaluated per index: no sort, no generator state, the same numbers on every device.
 * seed: basic.seed with the rank folded in by the caller; update: the caller's update counter; epoch: the mini-epoch (below 2^24).  perm: int32 [n]. */
int bg_perm_fill(int32_t n, uint64_t seed, uint32_t update, uint32_t epoch, int32_t* perm, void* stream);
/* One row-major fp32 stream of bg_gather_rows: dst [rows][width] = rows of src [src_rows][width]. */
typedef struct {
    const float* src;
    float* dst;
    int32_t width; /* floats per row, 1 to 4096; a multiple of 4 with 16-byte aligned buffers moves 16 bytes per thread */
    int32_t pad;
} bg_gather_stream;
#define BG_GATHER_MAX_STREAMS 8
/* dst_s[i][:] = src_s[perm[i]][:] for i < rows and every stream s < n_streams (1 to BG_GATHER_MAX_STREAMS), all in ONE launch: bit copies, no
 * arithmetic.  perm: int32 [rows] with values in [0, src_rows); a value outside leaves its destination row as it was (never read out of bounds).
 * A stream's src and dst must not overlap. */
int bg_gather_rows(int32_t rows, int32_t src_rows, const int32_t* perm, const bg_gather_stream* streams, int32_t n_streams, void* stream);

/* ---- env-wise mini-batches of sequences for PPO on a recurrent actor (runner.num_env_mini_batches > 1; bg_minibatch.hip).  One launch of its own
 * per mini-epoch (beside a bg_perm_fill over the envs): nothing of it runs when the key is absent or 1.
 *
 * One row-major stream of bg_gather_sequences.  per_env = 0: src [T][N][width] -> dst [K][T][n][width]; per_env != 0: src [N][width] -> dst
 * [K][n][width] (the recurrence's starting state). */
typedef struct {
    const void* src;
    void* dst;
    int32_t width;     /* elements per row, 1 to 4096; a row of a multiple of 16 bytes with 16-byte aligned buffers moves 16 bytes per thread */
    int32_t elem_size; /* bytes per element: 4, or 1 (the reset flags) */
    int32_t per_env;
    int32_t pad;
} bg_sequence_stream;
#define BG_SEQUENCE_MAX_STREAMS 12
/* With n = N / K (K must divide N) and sigma an int32 permutation of the envs [0, N): for every per-row stream
 *   dst[(k T + t) n + j][:] = src[t N + sigma[k n + j]][:],  k < K, t < T, j < n
 * -- mini-batch k holds the whole T-step sequences of its n envs, step-major -- and for every per-env stream dst[i][:] = src[sigma[i]][:], i < N; all
 * streams (1 to BG_SEQUENCE_MAX_STREAMS) in ONE launch: bit copies, no arithmetic.  A value of sigma outside [0, N) leaves its T destination rows
 * (its one per-env row) as they were and is never read out of bounds.  A stream's src and dst must not overlap; T x N stays below 2^31. */
int bg_gather_sequences(int32_t T, int32_t N, int32_t K, const int32_t* sigma, const bg_sequence_stream* streams, int32_t n_streams, void* stream);

const char* bg_last_error(void);
const char* bg_version(void);

#ifdef __cplusplus
}
#endif
#endif
