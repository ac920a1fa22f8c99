/*
 * hftlob.h — C ABI of the MI355X-native limit-order-book engine and the
 * multi-agent HFT environment step (libhftlob.so, HIP/gfx950).
 *
 * Every entry point takes plain pointers and sizes.  All array pointers are
 * DEVICE pointers (HBM) unless marked [host]; `stream` is a hipStream_t passed
 * as void* (NULL = the legacy default stream).  Nothing here allocates,
 * synchronises or talks to the host inside step/reset, so a caller may capture
 * these calls in a hipGraph.  Functions return 0 on success and a negative
 * HFTLOB_E* code on an invalid config / shape / null pointer; data conditions
 * never raise (the reference's silent semantics are reproduced:
 * -1 index wrap, book-full eviction, trade-log overwrite, slice clamping).
 *
 * Reference interfaces replaced (paths relative to biiiipy/JaxMARL-HFT):
 *   hftlob_book_process  <- jaxob/JaxOrderBookArrays.py:791-823
 *                           scan_through_entire_array_save_bidask(cfg, key,
 *                           msg_array, (asks,bids,trades), N_steps), vmapped;
 *                           with best_asks/best_bids == NULL it is
 *                           scan_through_entire_array (:736-756).
 *   hftlob_book_process_depth <- :758-789 scan_through_entire_array_save_states, vmapped, with
 *                           jaxob/jorderbook.py:122-135's get_L2_state of every saved state.
 *   hftlob_book_depth    <- :1231-1264 get_L2_state, vmapped.
 *   hftlob_env_reset     <- jaxen/marl_env.py:763-770 MARLEnv.reset ->
 *                           reset_env :129-207 (vmapped over envs).
 *   hftlob_env_step      <- jaxen/marl_env.py:775-804 MARLEnv.step (step_env
 *                           :211-709 + auto-reset select), vmapped over envs.
 *   hftlob_env_rollout_eval <- jaxrl/MARL/baseline_eval/baseline_only_JAXMARL.py: the scanned
 *                           _env_step with FixedAction policies and the reduction of its
 *                           trajectory batch (avg_reward, total_dones, info means / stds).
 *   hftlob_draw_actions / hftlob_env_rollout_eval_drawn <- the same scripts' multi-action FixedAction
 *                           (baseline_only_JAXMARL.py:58-71) and baseline_JAXMARL.py:367-374
 *                           RandomPolicy: an action drawn uniformly from a set at every step.
 *   hftlob_env_rollout_eval_episodes / hftlob_env_rollout_eval_drawn_episodes / hftlob_eval_tally_episodes
 *                        <- the per-episode reward arrays [episodes, agents] those evaluations feed to
 *                           baseline_eval/plotting_combinations.py (load_data), and the episodes' lengths
 *                           and end-of-episode info words beside them.
 *   hftlob_sample_actions<- jaxen/Speed_test.py:166-177 (per-env random actions
 *                           via gymnax Discrete.sample = jax.random.randint).
 *   hftlob_split_keys    <- jax.random.split(key, n) (threefry2x32), batched.
 *   hftlob_gru_scan_fwd / hftlob_gru_scan_bwd <- jaxrl/MARL/ippo_rnn_JAXMARL.py:53-78 ScannedRNN
 *                           (the nn.scan of a GRUCell whose carry is reset where done is set) and
 *                           its gradient through time, over a whole [T, B] sequence batch.
 *   hftlob_gru_scan_fwd_grouped / hftlob_gru_scan_bwd_grouped <- the same scans of several independent
 *                           nets (IPPO's one net per agent type) as one launch.
 *   hftlob_policy_step   <- jaxrl/MARL/ippo_rnn_JAXMARL.py:53-78, 183-256: one ActorCriticRNN step
 *                           (embedding, GRU cell, critic and actor heads) with the rollout's
 *                           pi.sample / log_prob (:590-600), for a batch of actors.
 *   hftlob_policy_step_multi <- the same step with :80-100 MultiActionOutputIndependant and :259-281
 *                           MultiCategorical: one categorical head per word of a MultiDiscrete space.
 *   hftlob_policy_step_grouped <- the same steps of several independent nets (IPPO's one net per agent
 *                           type; the runs of a sweep, :1274 wandb.agent) as one launch.
 *   hftlob_rollout_diag / hftlob_world_tally <- jaxrl/MARL/ippo_rnn_JAXMARL.py:977-1059, the update callback's
 *                           reductions of the trajectory batch (action shares, info means and stds).
 */
#ifndef HFTLOB_H
#define HFTLOB_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFTLOB_ABI_VERSION 8

#define HFTLOB_OK            0
#define HFTLOB_EINVAL      (-1)   /* bad config value / unsupported option */
#define HFTLOB_ENULL       (-2)   /* required pointer is NULL */
#define HFTLOB_ESHAPE      (-3)   /* size out of the supported range */
#define HFTLOB_ELAUNCH     (-4)   /* HIP launch error (see hftlob_last_error) */

#define HFTLOB_MAX_TYPES   4      /* agent types per env */
#define HFTLOB_MAX_AGENTS  32     /* agents per env, all types */
#define HFTLOB_MAX_SLOTS   256    /* nOrders and nTrades upper bound */
#define HFTLOB_MAX_MSGS    256    /* messages per step upper bound */
#define HFTLOB_MAX_OBS     16     /* observation width upper bound */
#define HFTLOB_INFO_WORLD_WORDS 14
#define HFTLOB_INFO_AGENT_WORDS 24
#define HFTLOB_L2_LEVELS   10     /* get_L2_state levels of world debug_mode (marl_env.py:646-651) */
#define HFTLOB_DEBUG_WORDS(n_trades) (4 * HFTLOB_L2_LEVELS + 8 * (n_trades))
#define HFTLOB_MAX_DEPTH_LEVELS 16 /* hftlob_book_depth / _process_depth: 4 * n_levels words live in one 64-lane row */

/* ---- engine configuration: JAXLOB_Configuration (jaxob_config.py:12-30) --- */
typedef struct hftlob_lob_cfg {
    int32_t maxint;                /* 2147483647 */
    int32_t init_id;               /* -2 */
    int32_t book_depth;            /* 10 */
    int32_t cancel_mode;           /* 0 STRICT_BY_ID, 1 INCLUDE_INITS, 2 RANDOM, 3 RANDOM_LARGE */
    int32_t type_4_interpretation; /* 0 IOC, 1 LIM, 2 MKT */
    int32_t check_book_fill;       /* bool */
    int32_t n_orders;              /* slots per book side (nOrders) */
    int32_t n_trades;              /* trade-log rows (nTrades) */
    int32_t prng_partitionable;    /* cancel_mode 2/3 draws: jax_threefry_partitionable (env cfg: equal to
                                      hftlob_env_cfg.prng_partitionable) */
} hftlob_lob_cfg;

/* ---- agent kinds and the option enums (jaxen/mm_env.py, jaxen/exec_env.py) */
enum { HFTLOB_AGENT_MM = 0, HFTLOB_AGENT_EXE = 1 };
enum { HFTLOB_MM_ACT_FIXED_QUANTS = 0, HFTLOB_MM_ACT_DIRECTIONAL = 1, HFTLOB_MM_ACT_BOB_RL = 2,
       HFTLOB_MM_ACT_BOB_STRATEGY = 3, HFTLOB_MM_ACT_AVST = 4, HFTLOB_MM_ACT_SPREAD_SKEW = 5,
       HFTLOB_MM_ACT_SIMPLE = 6 };
enum { HFTLOB_MM_OBS_BASIC = 0, HFTLOB_MM_OBS_ENGINEERED = 1, HFTLOB_MM_OBS_MESSAGES = 2 };
enum { HFTLOB_MM_REW_PORTFOLIO_VALUE = 0, HFTLOB_MM_REW_BUY_SELL_PNL, HFTLOB_MM_REW_COMPLEX,
       HFTLOB_MM_REW_ZERO_INV, HFTLOB_MM_REW_SPOONER, HFTLOB_MM_REW_SPOONER_DAMPED,
       HFTLOB_MM_REW_SPOONER_ASYM_DAMPED, HFTLOB_MM_REW_SPOONER_ASYM_DAMPED2,
       HFTLOB_MM_REW_SPOONER_SCALED, HFTLOB_MM_REW_DELTA_PORTFOLIO_VALUE };
enum { HFTLOB_PRICE_MID = 0, HFTLOB_PRICE_MID_AVG = 1, HFTLOB_PRICE_FAR_TOUCH = 2,
       HFTLOB_PRICE_NEAR_TOUCH = 3 };
enum { HFTLOB_INVPEN_NONE = 0, HFTLOB_INVPEN_LINEAR, HFTLOB_INVPEN_QUADRATIC,
       HFTLOB_INVPEN_THRESHOLD, HFTLOB_INVPEN_EXP4 };
enum { HFTLOB_EXE_ACT_FIXED_QUANTS_COMPLEX = 0, HFTLOB_EXE_ACT_SIMPLEST_CASE = 1, HFTLOB_EXE_ACT_FIXED_QUANTS_1MSG = 2,
       HFTLOB_EXE_ACT_TWAP = 3, HFTLOB_EXE_ACT_FIXED_PRICES = 4 };
enum { HFTLOB_EXE_OBS_ENGINEERED = 0, HFTLOB_EXE_OBS_BASIC = 1, HFTLOB_EXE_OBS_SIMPLEST_CASE = 2 };
enum { HFTLOB_EXE_REW_NORMAL = 0, HFTLOB_EXE_REW_FINISH_FAST = 1, HFTLOB_EXE_REW_SIMPLEST_CASE = 2 };
enum { HFTLOB_TASK_RANDOM = 0, HFTLOB_TASK_BUY = 1, HFTLOB_TASK_SELL = 2 };

/* One agent type (one entry of MultiAgentConfig.dict_of_agents_configs). */
typedef struct hftlob_agent_type_cfg {
    int32_t kind;                  /* HFTLOB_AGENT_* */
    int32_t n_agents;              /* number_of_agents_per_type[t] */
    int32_t trader_id0;            /* first trader id; agent i has trader_id0 - i */
    int32_t n_actions;
    int32_t n_msgs;                /* num_messages_by_agent */
    int32_t n_action_msgs;         /* num_action_messages_by_agent */
    int32_t obs_dim;
    int32_t action_space;          /* HFTLOB_MM_ACT_* / HFTLOB_EXE_ACT_* */
    int32_t observation_space;     /* HFTLOB_MM_OBS_* / HFTLOB_EXE_OBS_* */
    int32_t reward_function;       /* HFTLOB_MM_REW_* / HFTLOB_EXE_REW_* */
    int32_t normalize;
    int32_t time_delay_obs_act;
    int32_t fixed_quant_value;
    /* market maker */
    int32_t tenth_action_market;   /* tenth_action == "MarketOrder" */
    int32_t sell_buy_all_option;   /* must be 0 */
    int32_t fixed_action_setting;
    int32_t fixed_action;
    int32_t auto_liquidate_threshold;
    int32_t unwind_price_penalty;
    int32_t inv_penalty;           /* HFTLOB_INVPEN_* */
    int32_t reference_price;       /* HFTLOB_PRICE_* (MM: mid/mid_avg/far/near; EXE: mid/far) */
    int32_t unwind_price;          /* HFTLOB_PRICE_* (mid/mid_avg/far) */
    int32_t clip_reward;
    int32_t exclude_extreme_spreads;
    int32_t volume_traded_bonus;   /* 0 none, 1 market_share */
    float   auto_liquidate_alpha;
    float   inv_penalty_lambda;
    float   inv_penalty_quadratic_factor;
    float   inv_penalty_threshold;
    float   reward_scaling_quo;
    float   inventoryPnL_eta;
    float   inventoryPnL_gamma;
    float   rebate_bps;
    float   unrealizedPnL_lambda;
    /* execution */
    int32_t task;                  /* HFTLOB_TASK_* */
    int32_t task_size;
    int32_t n_ticks_in_book;
    int32_t doom_price_penalty;
    float   reward_lambda;
    /* constants the reference forms in Python double, then uses as weak f32 */
    float   rebate_factor;         /* rebate_bps / 10_000 */
    float   one_minus_eta;         /* 1 - inventoryPnL_eta */
    /* market-maker action-space parameters (mm_env.py:1123-1809) */
    int32_t bob_v0;                /* bobRL / bobStrategy base quantity */
    int32_t n_ticks_offset;        /* simple */
    int32_t simple_nothing_action; /* simple: 4-entry tables (else 3) */
    int32_t multiplier_type;       /* spread_skew: 0 "tick", 1 "spread" */
    float   spread_multiplier;     /* spread_skew */
    float   skew_multiplier;       /* spread_skew */
    float   avst_var;              /* AvSt avst_var_parameter */
    float   avst_k;                /* AvSt avst_k_parameter */
    float   avst_log_term[8];      /* AvSt: f32 log(1 + gamma_a / k) per action (host, correctly rounded) */
    /* execution: doom_price_penalty * tick_size when the config gives a non-integer penalty
       (a Python float: the far-touch price is then computed in f32, exec_env.py:1544,1569-1573) */
    int32_t doom_penalty_is_float;
    float   doom_penalty_f32;
    /* action words per agent in the actions buffer: 1 for a Discrete space; n_actions (1..4) for
       the EXE fixed_prices MultiDiscrete([fixed_quant_value] * n_actions) space (exec_env.py:2167-2171) */
    int32_t action_width;
} hftlob_agent_type_cfg;

/*
 * Environment configuration (World_EnvironmentConfig + MultiAgentConfig), and
 * the per-env state RECORD layout.  The host (hftlob/layout.py) fills every
 * field including the offsets; kernels read offsets from here.
 *
 * Per-env record, int32 words (floats stored bit-cast), stride rec_words:
 *   [off_asks]   asks  [n_orders][6]   ask_raw_orders
 *   [off_bids]   bids  [n_orders][6]   bid_raw_orders
 *   [off_trades] trades[n_trades][8]
 *   [off_loaded] init_time[2], window_index, max_steps_in_episode,
 *                start_index, step_counter                  (LoadedEnvState)
 *   [off_best_bids] best_bids [M][2]; [off_best_asks] best_asks [M][2]
 *   [off_world]  time[2], order_id_counter, mid_price(f32), delta_time(f32)
 *   [off_agents] per agent, type order: MM 5 words
 *                {posted_distance_bid, posted_distance_ask, inventory,
 *                 total_PnL(f32), cash_balance(f32)}; EXE 13 words
 *                {init_price(f32), task_to_execute, quant_executed,
 *                 is_sell_task, p_vwap, total_revenue, drift_return,
 *                 advantage_return, slippage_rm, price_adv_rm,
 *                 price_drift_rm, vwap_rm, trade_duration (f32)}
 * The init-state table (one row per data window) holds the first
 * init_rec_words words of the same layout (LoadedEnvState).
 */
typedef struct hftlob_env_cfg {
    hftlob_lob_cfg lob;
    int32_t n_data_msg;            /* n_data_msg_per_step (D) */
    int32_t n_msgs;                /* M = D + sum_t n_agents_t * n_msgs_t */
    int32_t n_action_msgs;         /* A = sum_t n_agents_t * n_action_msgs_t */
    int32_t n_cancel_msgs;         /* C = M - D - A */
    int32_t tick_size;
    int32_t ep_type;               /* 0 fixed_steps, 1 fixed_time (data rows past init_time[0] +
                                      episode_time are masked; EXE engineered obs has 15 fields) */
    int32_t episode_time;
    int32_t window_selector;       /* -1 random */
    int32_t n_windows;
    int32_t n_data_rows;           /* rows of the message-data array */
    int32_t placeholder_order_id;
    int32_t artificial_trader_id;
    int32_t artificial_order_id;
    int32_t order_id_counter_start;
    int32_t shuffle_action_messages;
    int32_t prng_partitionable;    /* 1: jax_threefry_partitionable=True (JAX>=0.5) */
    int32_t n_types;
    int32_t n_agents;              /* all types */
    int32_t obs_stride;            /* floats per agent row in the obs buffer */
    int32_t rec_words, init_rec_words;
    int32_t off_asks, off_bids, off_trades, off_loaded;
    int32_t off_best_bids, off_best_asks, off_world, off_agents;
    int32_t info_words;            /* words per env in the optional info buffer */
    int32_t action_words;          /* sum_t n_agents_t * action_width_t: int32 words per env of actions */
    /* set by the library before each env launch (a caller's value is ignored): the multiplier of
       the exact floor division by tick_size, ceil(2^(31+l) / tick_size), l = ceil(log2 tick_size) */
    uint32_t tick_magic;
    hftlob_agent_type_cfg types[HFTLOB_MAX_TYPES];
} hftlob_env_cfg;

/* Outputs of one batched step / reset.  obs/rewards/dones may not be NULL;
 * info, obs_raw and msgs may be NULL (skipped).  Layouts:
 *   obs      f32   [n_env][n_agents][obs_stride]   (agent order = type order)
 *   rewards  f32   [n_env][n_agents]
 *   done_all bool (uint8 0/1) [n_env]              dones["__all__"]
 *   dones    bool (uint8 0/1) [n_env][n_agents]    dones["agents"]
 *   info     32-bit words [n_env][info_words]: world info then one
 *            HFTLOB_INFO_AGENT_WORDS block per agent (ints, or f32 bit-cast;
 *            field map in hftlob/layout.py)
 *   obs_raw  32-bit words [n_env][n_agents][obs_stride] (step only): each agent's
 *            un-normalised observation of the stepped state, the reference's
 *            info["agents"][t]["obs_raw"] under save_raw_observations
 *            (marl_env.py:684-685: get_observation(..., normalize=False,
 *            flatten=False)), fields in sorted-key order, int32 fields as int32 and
 *            float32 fields as f32 bits (key / dtype map in hftlob/layout.py); not
 *            zeroed for done agents and taken before the auto-reset, as info is
 *   msgs     int32 [n_env][n_msgs][8] (step only): the step's combined message
 *            array [cancels; shuffled actions; data] as processed by the book —
 *            the MM "messages" observation (mm_env.py:2820-2821), and
 *            info["world"]["total_msgs"] under world debug_mode
 *   debug    int32 [n_env][HFTLOB_DEBUG_WORDS(n_trades)] (step only): world
 *            debug_mode's info (marl_env.py:645-656) of the stepped state, taken
 *            before the auto-reset as info is: words [0, 40) lob_state =
 *            get_L2_state(asks, bids, 10) (JaxOrderBookArrays.py:1231-1264: 10 rows
 *            [ask_p, ask_q, bid_p, bid_q], unique ask prices ascending with -1 read
 *            as maxint, unique bid prices descending, missing levels maxint /
 *            -maxint, negative volumes 0), then the step's trade log [n_trades][8]
 *            (info["world"]["trades"]) */
typedef struct hftlob_step_out {
    float*   obs;
    float*   rewards;
    uint8_t* done_all;
    uint8_t* dones;
    int32_t* info;
    int32_t* obs_raw;
    int32_t* msgs;
    int32_t* debug;
} hftlob_step_out;

int         hftlob_version(void);
const char* hftlob_last_error(void);

/* Batched order-book message processing (engine operator).
 * Replaces jax.vmap(scan_through_entire_array_save_bidask) —
 * gymnax_exchange/jaxob/JaxOrderBookArrays.py:791-823 — and, with NULL best
 * arrays, jax.vmap(scan_through_entire_array) — :736-756.
 * msgs      [n_env][n_msg][8]      message rows [type,side,q,p,oid,tid,s,ns]
 * asks,bids [n_env][n_orders][6]   in/out
 * trades    [n_env][n_trades][8]   in/out (caller initialises, e.g. all -1)
 * best_asks,best_bids [n_env][n_msg][2] out: (price, qty) after every message,
 *           NULL for both = scan_through_entire_array (no per-message output).
 * keys      uint32 [n_env][2]: the scan's `key` argument; message k draws from
 *           split(key, n_msg)[k] (get_random_id_match, :141-164).  Only read
 *           for cancel_mode 2/3; may be NULL otherwise. */
int hftlob_book_process(const hftlob_lob_cfg* cfg /*[host]*/, int n_env, int n_msg, const uint32_t* keys,
                        const int32_t* msgs, int32_t* asks, int32_t* bids, int32_t* trades,
                        int32_t* best_asks, int32_t* best_bids, void* stream);

/* Batched get_L2_state — replaces jax.vmap(get_L2_state) (JaxOrderBookArrays.py:1231-1264) of
 * n_env books in HBM, n_levels in 1..HFTLOB_MAX_DEPTH_LEVELS.
 * depth int32 [n_env][n_levels][4] = [ask_p, ask_q, bid_p, bid_q] per level: unique ask prices
 *       ascending with -1 read as maxint, unique bid prices descending, missing levels maxint /
 *       -maxint, the volume summed at the level's price, negative volumes 0. */
int hftlob_book_depth(const hftlob_lob_cfg* cfg /*[host]*/, int n_env, int n_levels,
                      const int32_t* asks, const int32_t* bids, int32_t* depth, void* stream);

/* The message scan with the book after every message — replaces
 * jax.vmap(scan_through_entire_array_save_states) (JaxOrderBookArrays.py:758-789), with the L2
 * view of jorderbook.process_orders_array_l2 (jorderbook.py:122-135) taken in the same launch.
 * Processes msgs exactly as hftlob_book_process does (asks / bids / trades updated in place,
 * keys as there).  For each of the last n_keep messages k (1 <= n_keep <= n_msg) it writes the
 * state after message k:
 * depth    [n_env][n_keep][n_levels][4]  (may be NULL: no L2 output; n_levels is then ignored)
 * all_asks [n_env][n_keep][n_orders][6], all_bids likewise (both or none).
 * At least one of the outputs must be given.  n_msg == 0 writes nothing. */
int hftlob_book_process_depth(const hftlob_lob_cfg* cfg /*[host]*/, int n_env, int n_msg, const uint32_t* keys,
                              const int32_t* msgs, int32_t* asks, int32_t* bids, int32_t* trades,
                              int n_levels, int n_keep, int32_t* depth,
                              int32_t* all_asks, int32_t* all_bids, void* stream);

/* Batched MARLEnv.reset — replaces jax.vmap(env.reset, (0, None)):
 * gymnax_exchange/jaxen/marl_env.py:763-770 (reset_env :129-207,
 * BaseLOBEnv.reset_env base_env.py:218-234).
 * keys uint32 [n_env][2]; state [n_env][rec_words].
 * msg_data [n_data_rows][8]; init_states [n_windows][init_rec_words]. */
int hftlob_env_reset(const hftlob_env_cfg* cfg /*[host]*/, int n_env, const uint32_t* keys,
                     const int32_t* msg_data, const int32_t* init_states,
                     int32_t* state, const hftlob_step_out* out /*[host] struct*/, void* stream);

/* Batched MARLEnv.step with auto-reset — replaces
 * jax.vmap(env.step, in_axes=(0, 0, 0, None)): marl_env.py:775-804 (step_env
 * :211-709).  keys uint32 [n_env][2]; actions int32 [n_env][action_words]: agent by agent in
 * type order, action_width words each (== [n_env][n_agents] when every space is Discrete). */
int hftlob_env_step(const hftlob_env_cfg* cfg /*[host]*/, int n_env, const uint32_t* keys,
                    const int32_t* actions, const int32_t* msg_data, const int32_t* init_states,
                    int32_t* state, const hftlob_step_out* out /*[host] struct*/, void* stream);

/* One Speed_test rollout step in a single launch — replaces the body of
 * _env_step in gymnax_exchange/jaxen/Speed_test.py:165-185:
 *   rng, *step_keys = split(rng, n_env + 1)      (key_in -> key_out, step keys)
 *   actions = hftlob_sample_actions(step_keys)     (written to actions_out if not NULL)
 *   hftlob_env_step(step_keys, actions, ...)
 * key_in / key_out: uint32 [2] device buffers, distinct (every env reads
 * key_in; key_out receives split(key_in, n_env + 1)[0]). */
int hftlob_env_step_sampled(const hftlob_env_cfg* cfg /*[host]*/, int n_env, const uint32_t* key_in,
                            uint32_t* key_out, int32_t* actions_out, const int32_t* msg_data,
                            const int32_t* init_states, int32_t* state, const hftlob_step_out* out /*[host] struct*/,
                            void* stream);

/* n_steps consecutive Speed_test rollout steps — replaces the whole
 * jax.lax.scan of Speed_test.py:186-196 (`rollout`): the same results, bit for
 * bit, as n_steps hftlob_env_step_sampled calls with key_out fed back as
 * key_in.  Env e of this call takes the step key
 * split(master, key_n + 1)[key_e0 + e + 1]: a call over the whole batch has
 * key_e0 = 0, key_n = n_env; a rank that owns envs [key_e0, key_e0 + n_env)
 * of a NUM_ENVS = key_n batch sharded over GPUs (ippo_rnn_JAXMARL_pmap.py:292-332)
 * passes its offset, so N ranks together replay the single-device rollout.
 * n_slices = 0: ONE kernel launch for all n_steps; every env (one wavefront)
 * runs its steps back to back with its own copy of the master-key chain, so no
 * step boundary waits for the batch's slowest env (for 100/100-slot books the
 * book also stays in LDS between steps; the last step stores it to `state`).
 * n_slices = 1..4: the envs are cut into n_slices contiguous slices, each stepped
 * by one launch per step: slice 0 on `stream`, the others on library-owned HIP
 * streams of the stream's device, forked from / joined back to it with events
 * (no host synchronisation), so one slice's slowest envs overlap the other
 * slices' next steps.
 * key_scratch: uint32 [n_slices][2][2] device scratch owned by the caller (each
 * slice's copy of the master-key chain; may be NULL for n_slices = 0); one buffer
 * per concurrent caller stream.
 * per_step != 0: out->{obs,rewards,done_all,dones,info} and actions_out hold a
 * leading [n_steps] dimension (step t at offset t * their per-step size);
 * per_step == 0: each step overwrites them (the scan discards them).  key_out
 * receives the master key after n_steps splits.  The slice streams are created
 * on first use; call hftlob_rollout_prepare before capturing a rollout in a
 * hipGraph.  If a launch fails, the slices already enqueued are still joined
 * back into `stream` before the error is returned. */
int hftlob_env_rollout_sampled(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int key_e0, int key_n, int n_steps,
                               const uint32_t* key_in, uint32_t* key_out, uint32_t* key_scratch,
                               int32_t* actions_out, const int32_t* msg_data, const int32_t* init_states,
                               int32_t* state, const hftlob_step_out* out /*[host] struct*/, int per_step,
                               int n_slices, void* stream);

/* n_steps consecutive MARLEnv.step calls with the caller's keys and actions in ONE persistent
 * launch: bit for bit the results of
 *   for t: hftlob_env_step(cfg, n_env, keys + t*n_env*2, actions + t*n_env*action_words, ...)
 * keys uint32 [n_steps][n_env][2]; actions int32 [n_steps][n_env][action_words] (read only).
 * per_step as in hftlob_env_rollout_sampled (out->{obs,rewards,done_all,dones,info,obs_raw,msgs,debug}
 * carry a leading [n_steps]; with per_step == 0 only the last step's outputs are written).
 * Every env (one wavefront) runs its steps back to back as in the n_slices = 0 launch above (for
 * 100/100-slot books the book stays in LDS between steps); there is no master-key chain and no env
 * slicing.  The kernel instantiation is chosen by the rule of the other env launches, so
 * hftlob_env_launch_info describes this entry point too, apart from key_batch (the step keys
 * are the caller's).  Like them it neither allocates nor synchronises and can be captured in a
 * hipGraph. */
int hftlob_env_rollout_actions(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int n_steps, const uint32_t* keys,
                               const int32_t* actions, const int32_t* msg_data, const int32_t* init_states,
                               int32_t* state, const hftlob_step_out* out /*[host] struct*/, int per_step,
                               void* stream);

/* Evaluation rollout — replaces the reset / step / reduce loop of
 * gymnax_exchange/jaxrl/MARL/baseline_eval/baseline_only_JAXMARL.py (make_eval: _env_step scanned
 * NUM_STEPS times, then the trajectory batch reduced to means and standard deviations): n_steps
 * MARLEnv.step calls in ONE persistent launch as hftlob_env_rollout_actions with per_step == 0
 * makes them, whose every step also folds the agents' rewards and info words into `stats`.
 * keys uint32 [n_steps][n_env][2]; actions int32 [n_steps][n_env][action_words], or with
 * actions_fixed != 0 ONE row [action_words] read for every env and step (the script's FixedAction).
 * The state after the call and `out` (the last step's outputs) are bit for bit those of
 * hftlob_env_rollout_actions with per_step == 0 over the same keys and the expanded actions; the
 * steps before the last build no observation and store no output.  n_env and n_steps must be >= 1.
 * stats double [n_env][n_agents][HFTLOB_EVAL_WORDS], in/out: the call ADDS to what it finds, so a
 * long evaluation can be cut into calls (zero it before the first).  Quantity q of an agent at a
 * step: q = 0 its reward as stored to `rewards`, q = 1 + k its info word k
 * (HFTLOB_INFO_AGENT_WORDS of them, taken before the auto-reset as `info` is; words the agent's
 * kind does not use are 0), each widened exactly: float words float -> double, int words int32 ->
 * double (the map per kind is INFO_MM / INFO_EXE of hftlob/layout.py).  Words of an agent's row:
 *   0              steps tallied
 *   1              episodes completed (steps whose done_all was set)
 *   2, 3           the running episode's reward sum and length (both 0 again after an episode end)
 *   4, 5           sum and sum of squares of the completed episodes' reward sums
 *   6, 7           sum and sum of squares of the completed episodes' lengths
 *   8+2q, 9+2q     (q = 0..24) sum and sum of squares of quantity q over all tallied steps
 *   58+2k, 59+2k   (k = 0..23) sum and sum of squares of info word k at each episode's last step
 * Every word is a plain sequential double sum in step order (no fused multiply-add; the square of a
 * widened float or int32 is exact), so a sequential float64 loop over per-step outputs gives the
 * same bits (hftlob/evaluate.py reduce_steps).  The kernel instantiation follows the rule of the
 * other env launches (hftlob_env_launch_info, apart from key_batch); the call neither allocates
 * nor synchronises and can be captured in a hipGraph. */
#define HFTLOB_EVAL_WORDS 106
int hftlob_env_rollout_eval(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int n_steps, const uint32_t* keys,
                            const int32_t* actions, int actions_fixed, const int32_t* msg_data,
                            const int32_t* init_states, int32_t* state, double* stats,
                            const hftlob_step_out* out /*[host] struct*/, void* stream);

/* Per-episode records — the arrays the reference's evaluation plots read
 * (baseline_eval/plotting_combinations.py: episode rewards [episodes, agents] per combination), which
 * the sums above cannot give back.  One record of HFTLOB_EPISODE_WORDS doubles per (env, agent,
 * completed episode), holding exactly the values the accumulators add at the episode's last step:
 *   0              the episode's reward sum (the double added to stats word 4)
 *   1              the episode's length (the double added to word 6)
 *   2+k            (k = 0..23) info word k at the episode's last step, widened as for words 58+2k
 * episodes double [n_env][n_agents][ep_cap][HFTLOB_EPISODE_WORDS].  The record of a step whose done_all
 * is set goes to index i = the agent's stats word 1 before that step's increment: the episodes
 * completed so far, what a given `stats` carried in included.  It is written iff 0 <= i < ep_cap; a slot
 * the call does not write is left untouched.  The index is word 1, so a run cut into calls carries
 * nothing beyond its `stats` and the same `episodes`, and overflow shows as word 1 > ep_cap.  No
 * counter of its own, no atomics: every record is the same bits on every call, and bit for bit what
 * hftlob/evaluate.py reduce_steps(max_episodes=) gives.
 * hftlob_env_rollout_eval_episodes is hftlob_env_rollout_eval with such a buffer: the same kernels (the
 * entry point without a buffer passes them none), the same state, `out` and `stats` bit for bit.  The
 * lanes of the env's wave that hold the values at the tally store them (26 stores per agent and
 * episode end).  HFTLOB_EINVAL: episodes NULL or ep_cap < 1; everything else is refused as
 * hftlob_env_rollout_eval refuses it. */
#define HFTLOB_EPISODE_WORDS 26
int hftlob_env_rollout_eval_episodes(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int n_steps, const uint32_t* keys,
                                     const int32_t* actions, int actions_fixed, const int32_t* msg_data,
                                     const int32_t* init_states, int32_t* state, double* stats,
                                     const hftlob_step_out* out /*[host] struct*/,
                                     double* episodes /*[n_env][n_agents][ep_cap][HFTLOB_EPISODE_WORDS]*/, int ep_cap,
                                     void* stream);

/* The accumulators above from per-step outputs, as one launch — replaces the reduction of the
 * trajectory batch in baseline_eval/baseline_JAXMARL.py (:819-951) for a caller whose actions do not
 * come from the env launch (a policy network: hftlob/evaluate.py evaluate_policy), and who therefore
 * holds each step's rewards, info record and global dones.
 * rewards float [n_steps][n_env][n_agents]; info int32 [n_steps][n_env][info_words], the raw record
 * of hftlob_step_out.info, agent a's words from HFTLOB_INFO_WORLD_WORDS + a * HFTLOB_INFO_AGENT_WORDS;
 * done_all bytes [n_steps][n_env] (non-zero: the step ended the env's episode).
 * float_words uint32 [n_agents], HOST: bit k set = info word k of that agent is a float, widened
 * float -> double; a clear bit widens the word int32 -> double (hftlob/evaluate.py _float_words gives
 * the map of a layout).  The array is read at the call and travels to the kernel by value.
 * stats double [n_env][n_agents][HFTLOB_EVAL_WORDS], in/out: the call ADDS the n_steps steps in order
 * to what it finds, the words as listed for hftlob_env_rollout_eval, every one a plain sequential
 * double sum of separately rounded terms (no fused multiply-add), so the result is bit for bit
 * hftlob/evaluate.py reduce_steps and, over the same steps, the stats of hftlob_env_rollout_eval; a
 * run cut into calls gives the bits of one call.
 * One lane per (env, agent, quantity): each stats word is read once and written once per launch;
 * no LDS, no atomics.  The call neither allocates nor synchronises and can be captured in a hipGraph.
 * HFTLOB_EINVAL: a NULL pointer; n_env, n_agents or n_steps < 1; n_agents > HFTLOB_MAX_AGENTS;
 * info_words < HFTLOB_INFO_WORLD_WORDS + n_agents * HFTLOB_INFO_AGENT_WORDS. */
int hftlob_eval_tally(int n_env, int n_agents, int n_steps, int info_words,
                      const float* rewards /*[n_steps][n_env][n_agents]*/,
                      const int32_t* info /*[n_steps][n_env][info_words]*/,
                      const uint8_t* done_all /*[n_steps][n_env]*/,
                      const uint32_t* float_words /*[n_agents], host*/,
                      double* stats /*[n_env][n_agents][HFTLOB_EVAL_WORDS], in/out*/, void* stream);

/* hftlob_eval_tally with the per-episode records of hftlob_env_rollout_eval_episodes (the same buffer,
 * the same index rule, the same bits): at a step with done_all set the lane of quantity q stores its
 * own word of the record (q = 0: words 0 and 1; q >= 1: word 1 + q).  Every lane counts the agent's
 * episodes itself from stats word 1, so no lane talks to another.  HFTLOB_EINVAL: episodes NULL or
 * ep_cap < 1; everything else is refused as hftlob_eval_tally refuses it. */
int hftlob_eval_tally_episodes(int n_env, int n_agents, int n_steps, int info_words,
                               const float* rewards /*[n_steps][n_env][n_agents]*/,
                               const int32_t* info /*[n_steps][n_env][info_words]*/,
                               const uint8_t* done_all /*[n_steps][n_env]*/,
                               const uint32_t* float_words /*[n_agents], host*/,
                               double* stats /*[n_env][n_agents][HFTLOB_EVAL_WORDS], in/out*/,
                               double* episodes /*[n_env][n_agents][ep_cap][HFTLOB_EPISODE_WORDS]*/, int ep_cap,
                               void* stream);

/* The drawn actions of a uniform baseline policy for a batch of actors, as one launch — replaces the
 * per-step pi.sample of the reference's multi-action FixedAction (baseline_eval/
 * baseline_only_JAXMARL.py:58-71, 305; baseline_JAXMARL.py:381-394: a distrax.Categorical with the same
 * probability on each listed action) and of its RandomPolicy (baseline_JAXMARL.py:367-374: uniform
 * over the action space), for a caller who steps the env himself (hftlob/evaluate.py evaluate_policy).
 * actions[b] is the smallest a with bit a of `allowed` set that maximises g[b][a], where
 * g = jax.random.gumbel(key, (n_actors, n_actions)) under the partitionable threefry in float32 (the
 * random word of element (b, a) is at counter (0, b * n_actions + a)): jax.random.categorical on logits
 * 0 on the allowed actions and -inf elsewhere.  A mask of exactly one bit draws nothing and gives that
 * action.  hftlob/evaluate.py draw_actions_reference is the definition on the CPU; the float32
 * logarithms may differ from the host's in the last place, so a row whose two largest allowed noises
 * are closer than that is not pinned.  (The reference adds log(1 / k) to the k allowed logits, which
 * moves no argmax but an exact float tie; no JAX-produced vector pins the draw.)
 * key uint32 [2] on the device.  32 lanes per actor: one threefry block and two logs per (b, a).
 * The call neither allocates nor synchronises and can be captured in a hipGraph.
 * HFTLOB_EINVAL: a NULL pointer; n_actors < 1; n_actions outside 1..32; an empty mask or mask bits
 * >= n_actions; n_actors * n_actions > 2^32 (the counter's low word). */
int hftlob_draw_actions(int n_actors, int n_actions, uint32_t allowed, const uint32_t* key /*[2], device*/,
                        int32_t* actions /*[n_actors]*/, void* stream);

/* hftlob_env_rollout_eval with the actions of uniform baseline policies drawn inside the launch: at
 * the top of every step each env's wave draws its own agents' action words.  Agent j of type i in env
 * e is actor b = e * n_agents_i + j of that type's n_env * n_agents_i actors, and its action at step t
 * is what hftlob_draw_actions gives actor b under draw_keys[t][i] and allowed[i].
 * draw_keys uint32 [n_steps][n_types][2], device; allowed uint32 [n_types], HOST, read at the call and
 * passed to the kernel by value (a mask of one bit is a fixed action); actions_out int32 [n_steps]
 * [n_env][action_words], device, receives the drawn words, NULL skips the stores.
 * The state, `out` and `stats` are bit for bit those of hftlob_env_rollout_eval over the same keys and
 * those [n_steps][n_env][action_words] actions.  The kernel instantiation follows the rule of the other
 * env launches (hftlob_env_launch_info, apart from key_batch); the call neither allocates nor
 * synchronises and can be captured in a hipGraph.
 * HFTLOB_EINVAL: prng_partitionable off (the draw is built for the partitionable threefry only); a
 * type with action_width != 1 (a MultiDiscrete space), n_actions outside 1..32, an empty mask or mask
 * bits >= n_actions; n_env * n_agents_i * n_actions_i > 2^32.  Sizes and NULL pointers are refused as
 * hftlob_env_rollout_eval refuses them. */
int hftlob_env_rollout_eval_drawn(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int n_steps, const uint32_t* keys,
                                  const uint32_t* draw_keys /*[n_steps][n_types][2]*/,
                                  const uint32_t* allowed /*[n_types], host*/,
                                  int32_t* actions_out /*[n_steps][n_env][action_words] or NULL*/,
                                  const int32_t* msg_data, const int32_t* init_states, int32_t* state, double* stats,
                                  const hftlob_step_out* out /*[host] struct*/, void* stream);

/* hftlob_env_rollout_eval_drawn with the per-episode records of hftlob_env_rollout_eval_episodes (the
 * same buffer, index rule and bits).  HFTLOB_EINVAL: episodes NULL or ep_cap < 1; everything else is
 * refused as hftlob_env_rollout_eval_drawn refuses it. */
int hftlob_env_rollout_eval_drawn_episodes(const hftlob_env_cfg* cfg /*[host]*/, int n_env, int n_steps,
                                           const uint32_t* keys, const uint32_t* draw_keys /*[n_steps][n_types][2]*/,
                                           const uint32_t* allowed /*[n_types], host*/,
                                           int32_t* actions_out /*[n_steps][n_env][action_words] or NULL*/,
                                           const int32_t* msg_data, const int32_t* init_states, int32_t* state,
                                           double* stats, const hftlob_step_out* out /*[host] struct*/,
                                           double* episodes /*[n_env][n_agents][ep_cap][HFTLOB_EPISODE_WORDS]*/,
                                           int ep_cap, void* stream);

/* Creates the library streams / events hftlob_env_rollout_sampled needs for n_slices
 * slices on the device of `stream` (host-only; idempotent). */
int hftlob_rollout_prepare(int n_slices, void* stream);

/* Dynamic LDS bytes of one env's workgroup in hftlob_env_step / hftlob_env_rollout_sampled
 * for this config (agent rows, action extras, book sides, trade log, pad / filter / scratch rows
 * and the rollout's step-key batches), or a negative HFTLOB_E* code for an invalid cfg
 * (host-only, no device call).  Hosts size launch shapes from it (how many envs a CU holds at
 * once); it replaces nothing in the reference, whose XLA compiler sizes its own buffers. */
int hftlob_env_lds_bytes(const hftlob_env_cfg* cfg /*[host]*/);

/* Which kernel instantiation hftlob_env_step / hftlob_env_rollout_sampled /
 * hftlob_env_rollout_actions / hftlob_env_rollout_eval / hftlob_env_rollout_eval_drawn launch for this config (key_batch: the
 * sampled rollout only), and
 * the launch-derived constants they pass it (host-only, no device call).  Tests use it to assert which code path a parity case ran; it replaces nothing in the reference.
 *   slot_sets     register sets per lane (1, 2 or 4: n_orders / n_trades up to 64 / 128 / 256)
 *   nfix          100: the 100/100-slot specialisation; 0: the general-size kernel
 *   random_cancel 1: the cancel_mode 2/3 (get_random_id_match) instantiation
 *   rows_alias    1: the agents' message rows live inside the trade log (the layout that
 *                 raises the envs a CU holds, e.g. Speed_test's [5, 5] agents)
 *   lds_bytes     dynamic LDS per env workgroup (hftlob_env_lds_bytes)
 *   tick_magic    the multiplier of the exact floor division by tick_size the kernels use,
 *                 ceil(2^(31+l) / tick_size), l = ceil(log2 tick_size)
 *   key_batch     1: hftlob_env_rollout_sampled's persistent launch derives the step keys four
 *                 steps at a time (partitionable keys, <= 3 agents, <= 8 action rows) */
typedef struct hftlob_launch_info {
    int32_t slot_sets, nfix, random_cancel, rows_alias, lds_bytes;
    uint32_t tick_magic;
    int32_t key_batch;
} hftlob_launch_info;
int hftlob_env_launch_info(const hftlob_env_cfg* cfg /*[host]*/, hftlob_launch_info* out /*[host]*/);

/* Baked configs.  The library holds the env configs the package ships (the JSON files of hftlob/configs, packed
 * by hftlob.layout.pack_env_cfg) as compile-time constants, and for some of them an instantiation
 * of hftlob_env_rollout_sampled's persistent kernel (n_slices = 0) that reads no config word at run
 * time: today the ids 0 (2_player_fq_fqc) and 1 (3_player_fq_fqc_dir).  A launch takes it only when
 * the caller's config equals the baked one in every word but n_windows and n_data_rows (the day's;
 * they stay run-time words) and tick_magic (the library's own); any difference, a tick_size other
 * than the builtin data's included, takes the general kernel.  The results are the same bit for bit
 * either way, and hftlob_env_launch_info describes both (the variant is the same).  It replaces
 * what jax.jit does for the reference, whose config is static Python data folded by XLA.
 *
 * hftlob_env_baked_id: the id (index in file-name order of the builtin configs) of the baked config
 * `cfg` equals, or -1: no such config, an invalid cfg, or the switch below is off (host-only).
 * hftlob_set_baked: process-wide switch, default on; on = 0 makes every launch take the general
 * kernels (A/B runs and tests).  Returns the previous setting. */
int hftlob_env_baked_id(const hftlob_env_cfg* cfg /*[host]*/);
int hftlob_set_baked(int on);

/* Speed_test action sampling (Speed_test.py:166-177, gymnax Discrete.sample):
 * for env e with step key k_e,
 * sub = split(k_e, n_types); per type t, agent i:
 * actions[e][agent] = randint(split(sub[t], n_agents_t)[i], 0, n_actions_t), or for
 * MultiDiscrete (from_JAXMARL/spaces.py:57-65) the action_width words
 * randint(split(sub[t], n_agents_t)[i], (width,), 0, fixed_quant_value).
 * actions int32 [n_env][action_words]. */
int hftlob_sample_actions(const hftlob_env_cfg* cfg /*[host]*/, int n_env, const uint32_t* keys,
                          int32_t* actions, void* stream);

/* Batched jax.random.split (threefry2x32; partitionable = jax_threefry_partitionable):
 * out[e][j] = split(keys[e], n)[j]; out [n_env][n][2]. */
int hftlob_split_keys(int n_env, int n, int partitionable, const uint32_t* keys,
                      uint32_t* out, void* stream);

/* Fused GRU sequence scan of the learner (ScannedRNN, jaxrl/MARL/ippo_rnn_JAXMARL.py:53-78), float32.
 * gi [T][B][3H] is the input projection x W_ih^T + b_ih in gate order (r, z, n), computed by the
 * caller over all T at once; w_hh [3H][H], b_hh [3H]; done [T][B] bytes (non-zero: the carry entering
 * step t is reset).  With h_prev(t) = done[t] ? 0 : (t ? hseq[t-1] : h0), step t is
 *     gh = h_prev(t) . w_hh^T + b_hh
 *     r = sigmoid(gi_r + gh_r)   z = sigmoid(gi_z + gh_z)   n = tanh(gi_n + r * gh_n)
 *     hseq[t] = (1 - z) * n + z * h_prev(t)
 * hseq [T][B][H].  gates, when not NULL, receives (r, z, n, gh_n) of every step as [T][B][4H] (four
 * blocks of H), which is what the backward operator reads; NULL skips those stores and changes no
 * bit of hseq.  One launch per scan: a workgroup owns 16 batch rows for all T steps, and no workgroup
 * waits on another.  H must be 64, 128 or 256 (else HFTLOB_ESHAPE); T >= 1, B >= 1 (rows past B in
 * the last 16-row tile are neither read nor written). */
int hftlob_gru_scan_fwd(int T, int B, int H, const float* gi, const float* h0 /*[B][H]*/, const uint8_t* done,
                        const float* w_hh, const float* b_hh, float* hseq, float* gates /* or NULL */,
                        void* stream);

/* The scan's gradient through time from d_hseq [T][B][H] and the forward's hseq and gates:
 * for t = T-1 .. 0, carry = 0 at the start,
 *     dh = d_hseq[t] + carry
 *     dn = dh * (1 - z) * (1 - n^2)     dz = dh * (h_prev(t) - n) * z * (1 - z)
 *     dr = dn * gh_n * r * (1 - r)
 *     d_gi[t] = (dr, dz, dn)            d_gh[t] = (dr, dz, dn * r)
 *     carry = done[t] ? 0 : dh * z + d_gh[t] . w_hh
 * and d_h0 [B][H] is the carry after t = 0.  d_gi [T][B][3H]; d_gh_n [T][B][H] is dn * r, so that
 * d_gh = (d_gi_r, d_gi_z, d_gh_n).  The weight and bias gradients are left to the caller, as one
 * GEMM and one reduction over all T: d_w_hh = d_gh[T B, 3H]^T . h_prev[T B, H], d_b_hh = sum d_gh.
 * The same sizes, launch shape and codes as the forward operator; no pointer may be NULL. */
int hftlob_gru_scan_bwd(int T, int B, int H, const float* d_hseq, const float* hseq, const float* gates,
                        const float* h0, const uint8_t* done, const float* w_hh, float* d_gi, float* d_gh_n,
                        float* d_h0, void* stream);

/* The two scan operators over up to HFTLOB_GRU_MAX_GROUPS independent sequence batches ("groups": in
 * IPPO, the minibatches of the agent types' nets) as one launch per direction.  The groups share T and
 * H; each has its own B, arrays and weights (two groups may name the same w_hh / b_hh), with the
 * layouts and meanings of the single-batch operators above.  groups is a host array that is read
 * during the call only: the table travels by value in the kernel arguments, so the call makes no copy
 * to the device and can be captured in a graph.  A workgroup owns one 16-row tile of one group; tiles
 * never straddle groups, each group's tiles start at its row 0, and the grid is the sum of the groups'
 * tile counts.  The per-tile arithmetic is that of hftlob_gru_scan_fwd / _bwd (one device function
 * serves both), so every group's outputs equal bit for bit what the single-batch operator gives for
 * that group alone, whatever the other groups and their order.
 * HFTLOB_ESHAPE: n_groups outside 1..HFTLOB_GRU_MAX_GROUPS, T < 1, a group with B < 1, H not 64, 128
 * or 256.  HFTLOB_ENULL: groups or any array of a group is NULL, except the forward's gates (NULL skips
 * that group's gate stores and changes no bit of its hseq).  Rows past a group's B are neither read out
 * of bounds nor written. */
#define HFTLOB_GRU_MAX_GROUPS 8
typedef struct {
    int B;
    const float *gi, *h0;
    const uint8_t* done;
    const float *w_hh, *b_hh;
    float *hseq, *gates /* or NULL */;
} hftlob_gru_fwd_group;
typedef struct {
    int B;
    const float *d_hseq, *hseq, *gates, *h0;
    const uint8_t* done;
    const float* w_hh;
    float *d_gi, *d_gh_n, *d_h0;
} hftlob_gru_bwd_group;
int hftlob_gru_scan_fwd_grouped(int T, int H, int n_groups, const hftlob_gru_fwd_group* groups /*[host]*/,
                                void* stream);
int hftlob_gru_scan_bwd_grouped(int T, int H, int n_groups, const hftlob_gru_bwd_group* groups /*[host]*/,
                                void* stream);

/* Fused recurrent policy step: one ActorCriticRNN step (jaxrl/MARL/ippo_rnn_JAXMARL.py:53-78 ScannedRNN's
 * cell, :183-256 SingleActionOutput and ActorCriticRNN) for a batch of B actors as one launch, float32.
 * The weights are a host struct of device pointers in torch's nn.Linear / nn.GRUCell layouts
 * ([out][in] rows; the GRU's gate order is r, z, n).  Per row b, with h_prev = done[b] ? 0 : h_in[b]:
 *     x      = relu(obs . w_embed^T + b_embed)
 *     gi     = x . w_ih^T + b_ih          gh = h_prev . w_hh^T + b_hh
 *     r = sigmoid(gi_r + gh_r)   z = sigmoid(gi_z + gh_z)   n = tanh(gi_n + r * gh_n)
 *     h      = (1 - z) * n + z * h_prev                     -> h_out
 *     value  = relu(h . w_c1^T + b_c1) . w_c2^T + b_c2
 *     logits = relu(h . w_a1^T + b_a1) . w_a2^T + b_a2
 *     action : mode 1 = the first argmax of logits
 *              mode 0 = the first argmax of logits + g
 *     log_prob = logits[action] - max - log(sum exp(logits - max))
 * the cell of hftlob_gru_scan_fwd.  g [B][A] is jax.random.gumbel(key, (B, A)) under the partitionable
 * threefry (jax_threefry_partitionable; the legacy form is not built): with bits = y0 ^ y1 of
 * threefry2x32(key, (0, b A + a)), f = bitcast((bits >> 9) | 0x3f800000) - 1,
 * u = max(tiny, f (1 - tiny) + tiny) (tiny: float32's smallest normal) and g = -log(-log(u)), so mode 0
 * is jax.random.categorical(key, logits), the reference's pi.sample(seed=_rng).  key is two device
 * words, read in mode 0 only (NULL is allowed in mode 1).
 * h_out may be h_in (in place).  logits [B][A] may be NULL, which changes no bit of the other outputs.
 * Sizes: H and FC each 64, 128 or 256; 1 <= D <= 64; 1 <= A <= 16; B >= 1, else HFTLOB_ESHAPE; a
 * required NULL pointer is HFTLOB_ENULL; a mode outside {0, 1}, or a w_ih, w_hh, w_c1, w_a1 or w_a2
 * that is not 16-byte aligned, is HFTLOB_EINVAL.  A workgroup owns 16 rows and waits on no other; rows
 * past B in the last tile are never written, and rows of w_a2 past A are never read.  The call never
 * allocates and never synchronises: it runs on the caller's stream and can be captured in a HIP graph
 * (the struct is copied at the call; the arrays it points to are read at every replay). */
typedef struct {
    const float *w_embed /*[FC][D]*/, *b_embed /*[FC]*/;
    const float *w_ih /*[3H][FC]*/, *b_ih /*[3H]*/, *w_hh /*[3H][H]*/, *b_hh /*[3H]*/;
    const float *w_c1 /*[FC][H]*/, *b_c1 /*[FC]*/, *w_c2 /*[1][FC]*/, *b_c2 /*[1]*/;
    const float *w_a1 /*[H][H]*/, *b_a1 /*[H]*/, *w_a2 /*[A][H]*/, *b_a2 /*[A]*/;
} hftlob_policy_weights;

int hftlob_policy_step(int B, int D, int FC, int H, int A, const hftlob_policy_weights* w /*[host]*/,
                       const float* obs /*[B][D]*/, const uint8_t* done /*[B]*/,
                       const float* h_in /*[B][H]*/, float* h_out /*[B][H]; may be h_in*/,
                       int mode, const uint32_t* key /*[2], device; mode 0 only*/,
                       int32_t* action /*[B]*/, float* log_prob /*[B]*/, float* value /*[B]*/,
                       float* logits /*[B][A] or NULL*/, void* stream);

/* hftlob_policy_step for a MultiDiscrete action space: the reference's MultiActionOutputIndependant and
 * MultiCategorical (ippo_rnn_JAXMARL.py:80-100, 259-281), K categorical heads on the shared relu(actor1)
 * features.  nvec [K] (host, read at the call; the offsets travel by value) holds the heads' sizes,
 * S = sum nvec; w_a2 is [S][H] and b_a2 [S], the heads' rows stacked in order, head k from row
 * off_k = nvec[0] + .. + nvec[k-1].  Everything up to relu(actor1) and value is hftlob_policy_step; then
 * per head k
 *     logits_k = relu(actor1) . w_a2[off_k : off_k + nvec[k]]^T + b_a2[off_k : off_k + nvec[k]]
 *     action[b][k] : mode 1 = the first argmax of logits_k, mode 0 = the first argmax of logits_k + g_k
 * with g_k [B][nvec[k]] the Gumbel draw of hftlob_policy_step from keys[k] at counter (0, b nvec[k] + a):
 * jax.random.categorical(keys[k], logits_k).  log_prob[b] is the sum over k = 0 .. K-1 of head k's
 * log-softmax at its action, added in float32 in that order.  The caller supplies
 * keys = jax.random.split(key, K) (hftlob_split_keys); with K == 1 the reference does not split, and the
 * call gives bit for bit what hftlob_policy_step gives with A = nvec[0] and key = keys[0].
 * Sizes: 1 <= K <= 4 and 1 <= nvec[k] <= 16, else HFTLOB_ESHAPE; B, D, FC, H, the NULL and alignment
 * rules, in-place h_out, the optional logits and graph capture are as for hftlob_policy_step. */
int hftlob_policy_step_multi(int B, int D, int FC, int H, int K, const int* nvec /*[K], host*/,
                             const hftlob_policy_weights* w /*[host]; w_a2 [S][H], b_a2 [S]*/,
                             const float* obs /*[B][D]*/, const uint8_t* done /*[B]*/,
                             const float* h_in /*[B][H]*/, float* h_out /*[B][H]; may be h_in*/,
                             int mode, const uint32_t* keys /*[K][2], device; mode 0 only*/,
                             int32_t* action /*[B][K]*/, float* log_prob /*[B]*/, float* value /*[B]*/,
                             float* logits /*[B][S] or NULL*/, void* stream);

/* The policy step of up to HFTLOB_POLICY_MAX_GROUPS independent nets ("groups": the agent types of an IPPO
 * run, or of several runs trained side by side) as one launch.  The groups share FC, H and mode; each has
 * its own B, D, heads (K of them, nvec[0 .. K-1] wide), weights and arrays, with the layouts and meanings
 * of hftlob_policy_step_multi: keys [K][2], action [B][K], logits [B][S] or NULL.  groups is a host array
 * that is read during the call only: the table travels by value in the kernel arguments, so the call
 * makes no copy to the device and can be captured in a graph.  A workgroup owns one 16-row tile of one
 * group; tiles never straddle groups, each group's tiles start at its row 0, and the grid is the sum of
 * the groups' tile counts.  The per-tile arithmetic is that of the single operators (one device function
 * serves all three), so every group's h_out, action, log_prob, value and logits equal bit for bit what
 * hftlob_policy_step_multi gives for that group alone (and so, for a group of one head, what
 * hftlob_policy_step gives with A = nvec[0] and key = keys), in both modes, whatever the other groups and
 * their order.  Per group h_out may be h_in; the outputs of different groups must not alias.  Rows past a
 * group's B are neither read out of bounds nor written.
 * HFTLOB_ESHAPE: n_groups outside 1..HFTLOB_POLICY_MAX_GROUPS; HFTLOB_ENULL: groups is NULL; then per
 * group, in group order, the checks of hftlob_policy_step_multi in their order and with its codes, the
 * message (hftlob_last_error) naming the group as "group g". */
#define HFTLOB_POLICY_MAX_GROUPS 8
typedef struct {
    int B, D, K;
    int nvec[4];
    hftlob_policy_weights w;
    const float* obs;
    const uint8_t* done;
    const float* h_in;
    float* h_out;
    const uint32_t* keys;
    int32_t* action;
    float *log_prob, *value, *logits /* or NULL */;
} hftlob_policy_group;
int hftlob_policy_step_grouped(int FC, int H, int n_groups, const hftlob_policy_group* groups /*[host]*/,
                               int mode, void* stream);

/* Generalised advantage estimation of the learner (_calculate_gae, ippo_rnn_JAXMARL.py:668-690) as one
 * launch, float32.  reward, value, adv, targets [T][n]; done bytes [T][n] (non-zero: the step ended the
 * episode); last_val [n].  One lane owns one actor and walks t = T-1 .. 0 with gae = 0 and
 * next_value = last_val at the start; with nd = 1.0f - done[t], every operation separately rounded:
 *     delta      = (reward[t] + (gamma * next_value) * nd) - value[t]
 *     gae        = delta + ((gamma_lambda * nd) * gae)
 *     adv[t]     = gae        targets[t] = gae + value[t]        next_value = value[t]
 * gamma and gamma_lambda are the caller's gamma and gamma * lambda (the product formed in double)
 * rounded to float32; the result is hftlob/train/ippo.py calculate_gae bit for bit.
 * HFTLOB_EINVAL: T or n < 1; HFTLOB_ENULL: a NULL pointer.  The call neither allocates nor synchronises,
 * runs on the caller's stream and can be captured in a HIP graph. */
int hftlob_gae(int T, int n, const float* reward, const float* value, const uint8_t* done,
               const float* last_val /*[n]*/, float gamma, float gamma_lambda, float* adv, float* targets,
               void* stream);

/* The PPO objective of the learner (_loss_fn, ippo_rnn_JAXMARL.py:718-765, under MultiCategorical,
 * :259-281) over N elements with its gradient, float32: hftlob/train/ippo.py ppo_loss_multi and what
 * autograd makes of it.  K heads of widths nvec[k] (host, read at the call; they travel by value),
 * S = sum nvec; logits [N][S], the heads side by side; actions int32 [N][K]; values, rb_value,
 * rb_log_prob, adv, targets [N].  Every actions[i][k] must lie in [0, nvec[k]); this is a precondition the
 * call does not check (a value outside it reads no memory out of bounds, but the result is undefined).
 * Per element, with mean and the population std of adv over the N elements
 * (accumulated in double):
 *     A = (adv - mean) / (std + 1e-8)
 *     lp_k = log_softmax(logits_k)   p_k = exp(lp_k)   H_k = -sum_j p_k[j] lp_k[j]
 *     logp = sum_k lp_k[a_k]   ent = sum_k H_k   lr = logp - rb_log_prob   ratio = exp(lr)
 *     a = ratio A              b = clamp(ratio, 1 - eps, 1 + eps) A
 *     u = v - tgt              c = rb_v + clamp(v - rb_v, -eps, eps) - tgt
 * out6 [6] (device) receives, as means over N,
 *     value_loss = 0.5 mean(max(u^2, c^2))   actor_loss = -mean(min(a, b))   entropy = mean(ent)
 *     approx_kl = mean((ratio - 1) - lr)     clip_frac = mean(|ratio - 1| > eps)
 * in the order total = actor_loss + vf_coef value_loss - ent_coef entropy, value_loss, actor_loss,
 * entropy, approx_kl, clip_frac.  d_logits [N][S] and d_values [N] receive the gradient of total for an
 * upstream gradient of 1, in torch's conventions (minimum / maximum split a tie evenly, clamp passes
 * the gradient on its inclusive bounds):
 *     w = 1 if a < b, 0 if a > b, at a == b 1/2 + 1/2 [1 - eps <= ratio <= 1 + eps]
 *     g_lp = -A w ratio / N
 *     d_logits_k[j] = g_lp ([j == a_k] - p_k[j]) + (ent_coef / N) p_k[j] (lp_k[j] + H_k)
 *     g_v = u if u^2 > c^2, c [-eps <= v - rb_v <= eps] if u^2 < c^2, half of each at equality
 *     d_values = vf_coef g_v / N
 * Both NULL: forward only, the same out6 bit for bit.  Three launches on the caller's stream (the
 * moments of adv; the element pass, HFTLOB_PPO_LOSS_ROWS elements per workgroup, which writes the
 * gradients and one row of partial sums per workgroup; the final sums), no floating-point atomic and a
 * fixed order of every sum: the same inputs give the same bits.  workspace is
 * HFTLOB_PPO_LOSS_WORKSPACE(N) doubles of the caller's, written before it is read.  The call neither
 * allocates nor synchronises and can be captured in a HIP graph.
 * HFTLOB_EINVAL: N < 1, K outside 1..4, an nvec[k] outside 1..16, exactly one of d_logits and d_values
 * NULL; HFTLOB_ENULL: any other NULL pointer. */
#define HFTLOB_PPO_LOSS_ROWS 64
#define HFTLOB_PPO_LOSS_WS_HEAD 128   /* doubles: the moment partial sums */
#define HFTLOB_PPO_LOSS_WS_ROW 5      /* doubles per workgroup of the element pass */
#define HFTLOB_PPO_LOSS_WORKSPACE(N) \
    (HFTLOB_PPO_LOSS_WS_HEAD + HFTLOB_PPO_LOSS_WS_ROW * (((long long)(N) + HFTLOB_PPO_LOSS_ROWS - 1) / HFTLOB_PPO_LOSS_ROWS))
int hftlob_ppo_loss(int N, int K, const int* nvec /*[K], host*/, const float* logits /*[N][S]*/,
                    const float* values, const int32_t* actions /*[N][K]*/, const float* rb_value,
                    const float* rb_log_prob, const float* adv, const float* targets, double clip_eps,
                    double vf_coef, double ent_coef, double* workspace, float* out6 /*[6], device*/,
                    float* d_logits /*[N][S] or NULL*/, float* d_values /*[N] or NULL*/, void* stream);

/* The learner's optimiser step for one net: clipping of the gradients by their global norm
 * (torch.nn.utils.clip_grad_norm_) and one Adam step (torch.optim.Adam, capturable: the step counters are
 * float32 device scalars, lr is a float32 device scalar), float32, over up to HFTLOB_ADAM_MAX_TENSORS
 * parameter tensors.  No weight decay, no amsgrad, no maximize.  tensors is a host array, read at the
 * call: its pointers and sizes travel to the kernels by value, so they may differ from call to call and
 * nothing is copied to the device.  Per tensor: p, m (exp_avg), v (exp_avg_sq) [n], updated in place;
 * g [n], read only (the one difference from clip_grad_norm_, which scales the gradients in place);
 * step, one float, incremented by 1 before it is used.  Two launches on the caller's stream:
 *   the norm pass: at most HFTLOB_ADAM_NORM_BLOCKS workgroups walk the chunks of HFTLOB_ADAM_CHUNK
 *     elements (a tensor's chunks are its own, its last one may be short) in a fixed assignment, sum
 *     g^2 in double and leave one partial sum each in the workspace; workgroup 0 increments every step;
 *   the update pass: one workgroup per chunk.  Each folds the partial sums in the same order, and with
 *       total_norm = sqrt(sum g^2)          coef = min(1, max_norm / (total_norm + 1e-6))
 *       bc1 = 1 - beta1^step                bc2 = 1 - beta2^step          (the tensor's own step)
 *       step_size = lr / bc1                (these scalars in double, each rounded to float32 once)
 *     applies, every operation a separately rounded float32 one, with gc = g coef:
 *       m = m + (gc - m) (1 - beta1)        v = v beta2 + (1 - beta2) (gc gc)
 *       p = p - step_size (m / (sqrt(v) / sqrt(bc2) + eps))
 * No floating-point atomic and a fixed order of every sum: the same inputs give the same bits.
 * Non-finite gradients propagate as in torch (a NaN norm gives NaN parameters); nothing is checked.
 * beta1 and beta2 are doubles, as torch holds them: 1 - beta2 formed from a float32 0.999 is off by
 * 1.3e-5 of itself, which exp_avg_sq would inherit.  total_norm (device, one float) receives the norm
 * before clipping; it may be NULL.  workspace is HFTLOB_ADAM_WORKSPACE doubles of the caller's, written
 * before it is read.  The call neither allocates nor synchronises and can be captured in a HIP graph.
 * HFTLOB_ESHAPE: n_tensors outside 1..HFTLOB_ADAM_MAX_TENSORS, an n < 1 (or more than 2^31 - 1 chunks in
 * all); HFTLOB_ENULL: a NULL tensors, p, g, m, v, step, lr or workspace; HFTLOB_EINVAL: max_norm not finite
 * or <= 0, a beta outside [0, 1), eps < 0 (or not finite), a p, g, m or v that is not 16-byte aligned. */
#define HFTLOB_ADAM_MAX_TENSORS 16
#define HFTLOB_ADAM_CHUNK 1024        /* elements per workgroup of the update pass */
#define HFTLOB_ADAM_NORM_BLOCKS 64    /* the most workgroups of the norm pass */
#define HFTLOB_ADAM_WORKSPACE HFTLOB_ADAM_NORM_BLOCKS   /* doubles: one partial sum per workgroup */
typedef struct {
    float* p;          /* [n] the parameter, in/out */
    const float* g;    /* [n] its gradient, read only */
    float* m;          /* [n] exp_avg, in/out */
    float* v;          /* [n] exp_avg_sq, in/out */
    float* step;       /* one float, in/out: the steps taken */
    long long n;
} hftlob_adam_tensor;
int hftlob_adam_clip(int n_tensors, const hftlob_adam_tensor* tensors /*[n_tensors], host*/,
                     const float* lr /*device, one float*/, double beta1, double beta2, float eps,
                     float max_norm, double* workspace /*HFTLOB_ADAM_WORKSPACE doubles*/,
                     float* total_norm /*device, one float, or NULL*/, void* stream);

/* The weight and bias gradients of the learner's narrow layers: a product reduced over many rows into a
 * small output, float32, row-major, contiguous,
 *       C[P][Q]  = sum_n A[n][p] B[n][q]          A [N][P], B [N][Q]
 *       sum_a[P] = sum_n A[n][p]                  (NULL to skip)
 *       sum_b[Q] = sum_n B[n][q]                  (NULL to skip)
 * for 1 <= P <= HFTLOB_XTY_MAX_P (any value), Q 64, 128 or 256, N >= 0.  For a linear layer y = x W^T + b
 * with a narrow output (W [P][Q]) A = d_y, B = x give d_W = C and d_b = sum_a; with a narrow input
 * (W [Q][P]) A = x, B = d_y give d_W = C^T and d_b = sum_b.  Two launches on the caller's stream:
 *   the partial pass cuts the rows into G contiguous stripes, one per workgroup (and per 16 rows of C).
 *     The stripe rule is a function of N alone, with R = HFTLOB_XTY_STRIPE_ROWS, M = HFTLOB_XTY_MAX_STRIPES:
 *         rows = R if ceil(N / R) <= M, else ceil(N / M)        G = ceil(N / rows)
 *     stripe g is the rows [g rows, min(N, (g + 1) rows)): up to M stripes of R rows, and past M R rows
 *     the stripes grow instead of their number; none is empty.  Inside a stripe each of a workgroup's four
 *     waves takes every fourth row and adds a[p] b[q] with one fused multiply-add (fmaf) per row, in row
 *     order; the four sums are added in wave order.  The workgroup leaves its float32 partial in the
 *     workspace: per stripe P Q + P + Q floats, [P][Q] of C, then sum_a's, then sum_b's (the sums' only
 *     when asked for);
 *   the final pass adds the G partials of every output element in double, in stripe order inside each of
 *     16 consecutive groups of ceil(G / 16) stripes, then the 16 group sums in group order, and rounds
 *     once to float32.
 * No floating-point atomic and a fixed order of every sum: the same inputs give the same bits on every
 * call, eager or replayed from a HIP graph, and C's bits do not depend on which sums are asked for.
 * Rows past N and columns past P or Q are never read.  workspace is the caller's, hftlob_xty_workspace(N,
 * P, Q) floats (G (P Q + P + Q); a host-only function that makes no device call), written before it is
 * read.  N = 0 zero-fills C and the sums that are not NULL with asynchronous memsets and reads nothing: A, B
 * and workspace may then be NULL.  The call neither allocates nor synchronises and can be captured in a HIP
 * graph.  Checked in this order, before any device work: HFTLOB_ESHAPE: P outside 1..HFTLOB_XTY_MAX_P, Q not
 * 64, 128 or 256, N < 0 (hftlob_xty_workspace returns the same code, as a negative size); HFTLOB_ENULL: a NULL
 * C, or with N > 0 a NULL A, B or workspace; HFTLOB_EINVAL: with N > 0 a B that is not 16-byte aligned. */
#define HFTLOB_XTY_MAX_P 64
#define HFTLOB_XTY_STRIPE_ROWS 128    /* R: the rows of a stripe up to HFTLOB_XTY_MAX_STRIPES stripes */
#define HFTLOB_XTY_MAX_STRIPES 512    /* M: the most stripes (workgroups per 16 rows of C) */
long long hftlob_xty_workspace(long long N, int P, int Q);   /* floats; < 0: an error code */
int hftlob_xty(long long N, int P, int Q, const float* A /*[N][P]*/, const float* B /*[N][Q]*/,
               float* C /*[P][Q]*/, float* sum_a /*[P] or NULL*/, float* sum_b /*[Q] or NULL*/,
               float* workspace, void* stream);

/* The weight and bias gradients of the learner's wide layers: the same product for a wide output, float32,
 *       C[P][Q]  = sum_n A[n][p] B'[n][q]         row-major, contiguous
 *       sum_a[P] = sum_n A[n][p]                  (NULL to skip)
 * for P a multiple of 64 in 64..HFTLOB_XTY_WIDE_MAX_P, Q 64, 128 or 256, N >= 0.  For a linear layer y = x W^T
 * + b (W [P][Q]) A = d_y, B = x give d_W = C and d_b = sum_a.
 *   A is one or two column blocks side by side, P = cols0 + cols1: block i is (Ai, colsi, stridei), row n of
 *     it the colsi floats at Ai + n stridei.  colsi is a multiple of 64 (cols1 = 0: one block, A1 is not
 *     looked at), stridei >= colsi and a multiple of 4, Ai 16-byte aligned.
 *   B' is B [N][Q] (contiguous, 16-byte aligned) behind a head and under a row mask:
 *         B'[n] = zero_row[n] ? 0 : (n < shift ? head[n] : B[n - shift])
 *     head is [shift][Q] (16-byte aligned; NULL: those rows are 0), zero_row N bytes (NULL: no mask), 0 <=
 *     shift <= N.  Rows N - shift .. of B are never read, nor is a masked row's value used (it may be NaN).
 *     With shift = the batch size, head = h0, B = hseq and zero_row = done, B' is the h_prev of
 *     hftlob_gru_scan_bwd's W_hh gradient, and A = (d_gi with cols 2H and stride 3H, d_gh_n) its d_gh.
 * Two launches on the caller's stream:
 *   the partial pass cuts the rows into G contiguous stripes and C into tiles of HFTLOB_XTY_WIDE_TILE_P rows
 *     by TQ columns, TQ = 64 for Q = 64 and 128 otherwise; one workgroup per stripe and tile.  The stripe
 *     rule is a function of (N, P, Q), with R = HFTLOB_XTY_WIDE_STRIPE_ROWS, tiles = ceil(P / 128) (Q / TQ)
 *     and M = ceil(HFTLOB_XTY_WIDE_TARGET_WGS / tiles):
 *         rows = R if ceil(N / R) <= M, else ceil(N / M)        G = ceil(N / rows)
 *     stripe g is the rows [g rows, min(N, (g + 1) rows)): up to M stripes of R rows, and past M R rows the
 *     stripes grow instead of their number; none is empty.  A workgroup walks its stripe in chunks of
 *     HFTLOB_XTY_WIDE_CHUNK rows and adds a[p] b[q] in row order with float32 matrix instructions whose
 *     result is that of one fused multiply-add (fmaf) per row; sum_a's partial is a float32 sum in row order.
 *     It leaves its float32 partial in the workspace: per stripe P Q + P floats, [P][Q] of C, then sum_a's
 *     (only when asked for);
 *   the final pass adds the G partials of every output element in double, in stripe order, and rounds once
 *     to float32.
 * No floating-point atomic and a fixed order of every sum: the same inputs give the same bits on every
 * call, eager or replayed from a HIP graph, and C's bits do not depend on whether sum_a is asked for, nor on
 * how A is cut into blocks or whether B' is given shifted and masked or materialised.  Rows past N are
 * never read.  workspace is the caller's, hftlob_xty_wide_workspace(N, P, Q) floats (G (P Q + P); a host-only
 * function that makes no device call), written before it is read.  N = 0 zero-fills C and sum_a (if not NULL)
 * with asynchronous memsets and reads nothing: every other pointer may then be NULL.  The call neither
 * allocates nor synchronises and can be captured in a HIP graph.  Checked in this order, before any device
 * work: HFTLOB_ESHAPE: cols0 not a multiple of 64 in 64..768, cols1 not 0 or such a multiple, P > 768, Q not
 * 64, 128 or 256, N < 0 (hftlob_xty_wide_workspace returns the same code for its P, Q and N, as a negative
 * size), shift outside 0..N; HFTLOB_ENULL: a NULL C, or with N > 0 a NULL A0, A1 (cols1 > 0), B (shift < N) or workspace;
 * HFTLOB_EINVAL: with N > 0 an A0, A1, B or head that is not 16-byte aligned, then a stride below its block's
 * columns or not a multiple of 4. */
#define HFTLOB_XTY_WIDE_MAX_P 768
#define HFTLOB_XTY_WIDE_TILE_P 128        /* rows of C in a workgroup's tile */
#define HFTLOB_XTY_WIDE_CHUNK 32          /* rows of A and B in a chunk */
#define HFTLOB_XTY_WIDE_STRIPE_ROWS 256   /* R: the rows of a stripe up to M stripes */
#define HFTLOB_XTY_WIDE_TARGET_WGS 512    /* M tiles >= this: two workgroups on each of 256 CUs */
long long hftlob_xty_wide_workspace(long long N, int P, int Q);   /* floats; < 0: an error code */
int hftlob_xty_wide(long long N, int Q, const float* A0, int cols0, long long stride0, const float* A1, int cols1,
                    long long stride1, const float* B /*[N][Q]*/, const float* head /*[shift][Q] or NULL*/,
                    long long shift, const unsigned char* zero_row /*[N] or NULL*/, float* C /*[P][Q]*/,
                    float* sum_a /*[P] or NULL*/, float* workspace, void* stream);

/* The training diagnostics: one agent type's rollout buffers reduced to HFTLOB_DIAG_WORDS doubles.  N = T *
 * n_actors elements, every array contiguous: action int32 [N][K] (K heads, head k of nvec[k] actions; the
 * limits are hftlob_ppo_loss's, 1 <= K <= HFTLOB_DIAG_MAX_HEADS and 1 <= nvec[k] <= HFTLOB_DIAG_MAX_ACTIONS),
 * reward, value, log_prob, adv, target float32 [N], done bytes [N] (the env's global done).  Words of diag:
 *    0          N
 *    1          the number of set (nonzero) done bytes
 *    2 + 2q     the sum of quantity q over the N elements, q = 0 reward, 1 value, 2 log_prob, 3 advantage,
 *    3 + 2q     4 target, 5 residual = (double)target - (double)value; and the sum of its squares
 *   14 + k      the sum of head k's action words that lie in [0, nvec[k])
 *   18 + k      the count of head k's action words outside [0, nvec[k]) (in no bin, not in the sum)
 *   22 + 16k + a   the count of head k's action a
 * Every value is widened to double before it is subtracted, squared or added; a square is one rounded double
 * product, added separately (no fused multiply-add).  Words of heads k >= K and of actions a >= nvec[k] are 0.
 * Two launches on the caller's stream:
 *   the partial pass cuts the elements into G contiguous stripes, one per workgroup of 256 lanes.  The stripe
 *     rule is a function of N alone, with R = HFTLOB_DIAG_STRIPE_ROWS, M = HFTLOB_DIAG_MAX_STRIPES:
 *         rows = R if ceil(N / R) <= M, else ceil(N / M)        G = ceil(N / rows)
 *     stripe g is the elements [g rows, min(N, (g + 1) rows)): up to M stripes of R elements, and past M R
 *     elements the stripes grow instead of their number; none is empty.  Lane l starts every one of the
 *     twelve words 2..13 at +0.0 and adds the stripe's elements begin + l, begin + l + 256, ... in that
 *     order; the stripe's partial of a word is the 256 lanes' sums added in lane order, from lane 0's (a
 *     lane without an element contributes its +0.0).  The counts are integers, exact in any order.  The
 *     workgroup leaves its partial of HFTLOB_DIAG_WORDS doubles in the workspace;
 *   the final pass adds the G partials of every word in stripe order, from stripe 0's.
 * No floating-point atomic and a fixed order of every sum: the same inputs give the same bits on every call,
 * eager or replayed from a HIP graph.  Elements past N are never read.  workspace is the caller's,
 * hftlob_rollout_diag_workspace(N) doubles (G HFTLOB_DIAG_WORDS; a host-only function that makes no device
 * call), written before it is read.  N = 0 zero-fills diag with an asynchronous memset and reads nothing: the
 * arrays and workspace may then be NULL.  The call neither allocates nor synchronises and can be captured in
 * a HIP graph.  Checked in this order, before any device work: HFTLOB_ESHAPE: N < 0
 * (hftlob_rollout_diag_workspace returns the same code, as a negative size), K outside
 * 1..HFTLOB_DIAG_MAX_HEADS; HFTLOB_ENULL: a NULL nvec or diag, or with N > 0 a NULL array or workspace;
 * HFTLOB_EINVAL: an nvec entry outside 1..HFTLOB_DIAG_MAX_ACTIONS.  hftlob/train/diag.py restates it in torch
 * (rollout_diag_reference). */
#define HFTLOB_DIAG_MAX_HEADS 4
#define HFTLOB_DIAG_MAX_ACTIONS 16
#define HFTLOB_DIAG_WORDS 86
#define HFTLOB_DIAG_STRIPE_ROWS 1024   /* R: the elements of a stripe up to HFTLOB_DIAG_MAX_STRIPES stripes */
#define HFTLOB_DIAG_MAX_STRIPES 256    /* M: the most stripes (workgroups of the partial pass) */
long long hftlob_rollout_diag_workspace(long long N);   /* doubles; < 0: an error code; host only */
int hftlob_rollout_diag(long long N, int K, const int* nvec /*[K], host*/,
                        const int32_t* action /*[N][K]*/, const float* reward, const float* value,
                        const float* log_prob, const float* adv, const float* target /*[N] each*/,
                        const uint8_t* done /*[N]*/, double* diag /*[HFTLOB_DIAG_WORDS], written*/,
                        double* workspace, void* stream);

/* The world half of hftlob_eval_tally: the world info words (the first HFTLOB_INFO_WORLD_WORDS words of an
 * env's info record) of n_steps steps folded into per-env sums.  info int32 [n_steps][n_env][info_words] as
 * the step launches write hftlob_step_out.info; float_words: bit k set = world word k is a float32 (it is
 * widened from the float with the word's bits, else from the int32).  wstats double
 * [n_env][HFTLOB_WORLD_TALLY_WORDS], in/out: word 2k receives the sum of world word k over the steps, in
 * step order, word 2k + 1 the sum of its squares (one rounded double product each, added separately), both
 * ADDED to what the call finds.  One lane per (env, word), sequential over the steps: bit for bit a float64
 * loop (hftlob/train/diag.py world_tally_reference).  One launch on the caller's stream; the call neither
 * allocates nor synchronises and can be captured in a HIP graph.  Checked in this order, before any device
 * work: HFTLOB_ESHAPE: n_env < 1, n_steps < 1, info_words < HFTLOB_INFO_WORLD_WORDS; HFTLOB_ENULL: a NULL
 * info or wstats; HFTLOB_EINVAL: a bit of float_words at or above HFTLOB_INFO_WORLD_WORDS. */
#define HFTLOB_WORLD_TALLY_WORDS 28   /* 2 * 14 world info words */
int hftlob_world_tally(int n_env, int n_steps, int info_words, const int32_t* info /*[n_steps][n_env][info_words]*/,
                       uint32_t float_words /*bit k: world word k is a float*/,
                       double* wstats /*[n_env][HFTLOB_WORLD_TALLY_WORDS], in/out*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HFTLOB_H */
