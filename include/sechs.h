/*
 * sechs.h -- C ABI of libsechs.so, the MI355X-native vectorised 6 nimmt!
 * engine (environment + random-policy self-play + Monte-Carlo search).
 *
 * The reference (coolo/rl-6-nimmt) is pure Python and has no FFI: its hot
 * path sits behind duck-typed Python interfaces.  Each entry point below
 * names the reference interface it replaces; the Python package
 * rl-6-nimmt_amd/rl_6_nimmt binds them with ctypes and
 * re-exposes the reference API (SechsNimmtEnv, GameSession, Tournament,
 * DrunkHamster, MCSAgent, ...).
 *
 * Conventions
 *  - No exceptions cross the ABI: every call returns sn_status; the text of
 *    the last error on the calling thread is sn_last_error().
 *  - The engine owns its device state.  The caller owns every I/O buffer;
 *    I/O pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr() of a
 *    cuda tensor) unless the parameter name ends in _host.
 *  - `stream` is a hipStream_t (NULL = the default stream).  Calls only
 *    enqueue work; they never synchronise the stream, except those marked
 *    [sync] (host-side state exchange).
 *  - One handle per device; no internal locking.  Several handles on
 *    several GPUs (one process per GPU) are independent.
 *  - Game g of a handle has the global id game_offset + g; every random
 *    stream is keyed by the global id, so results do not depend on how the
 *    games are sharded over handles / ranks.
 *  - Layouts are row-major, game-major: obs [B][N][obs_stride] etc.
 */
#ifndef SECHS_H
#define SECHS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sn_env sn_env; /* opaque */

typedef enum {
    SN_OK = 0,
    SN_EINVAL = 1,       /* bad argument (reference: AssertionError, env.py:19-21,67) */
    SN_EHIP = 2,         /* HIP runtime error */
    SN_ENOMEM = 3,       /* device allocation failed */
    SN_EUNSUPPORTED = 4, /* valid in the reference but not built here */
    SN_ERNG = 5,         /* a pipelined numpy-MT draw ran past the twisted words (sticky: every
                            rollout of this handle since then is invalid; see sn_pipe_errors) */
} sn_status;

/* random word sources; both drive numpy's legacy masked-rejection
   random_interval, so the draw structure is the reference's */
enum {
    SN_RNG_PHILOX = 0,   /* counter-based Philox4x32-10 keyed (seed, global game id) */
    SN_RNG_NUMPY_MT = 1, /* numpy legacy RandomState per game, seeded seed + global game id:
                            game g replays np.random.seed(seed+g) + GameSession(DrunkHamster x N) */
};

/* observation element types for sn_obs */
enum { SN_I8 = 1, SN_I16 = 2, SN_I32 = 3, SN_I64 = 4, SN_F32 = 5 };

/* sn_rollout / sn_step flags */
enum {
    SN_AUTO_RESET = 1,       /* a finished game is re-dealt at once from its own stream */
    SN_NO_SUMMARIES = 2,     /* obs without the 12 row summaries (include_summaries=False) */
};

const char* sn_last_error(void);
const char* sn_version(void);

/* SechsNimmtEnv.__init__ (env.py:16-41) for B games at once.
   num_players 1..10, num_cards 10*N+4 .. 104 (env.py:19-21; cards >= 104
   fail the reference's own _card_value assertion, env.py:228).
   num_rows / threshold are fixed at the reference defaults 4 / 6. */
sn_status sn_create(sn_env** out, int device, int64_t num_games, int num_players, int num_cards, uint64_t seed,
                    uint64_t game_offset, int rng_mode);
sn_status sn_destroy(sn_env* env);
sn_status sn_info(const sn_env* env, int64_t* num_games, int* num_players, int* num_cards, int* rng_mode);

/* env.py:43-51 reset() -> _deal() (:99-112).  decks == NULL: every game
   shuffles arange(C) from its own stream (np.random.shuffle); else decks
   is [B][C] uint8, one permutation per game.  Scores are zeroed. */
sn_status sn_reset(sn_env* env, const uint8_t* decks, void* stream);

/* env.py:53-62 reset_to(board, hands): board [B][4][6] int8 (row cards,
   -1 padded, 1..5 cards per row), hands [B][N][10] int8 (-1 padded, every
   seat holding the same count).  Scores are zeroed.  Inputs are copied. */
sn_status sn_reset_to(sn_env* env, const int8_t* board, const int8_t* hands, void* stream);

/* env.py:64-77 step(action).  actions [B][N] int32 (NULL = the in-kernel
   DrunkHamster policy, agents/random.py:8-10, drawn in seat order from each
   game's stream).  Outputs: rewards [B][N] int32 (<= 0), done [B] uint8,
   invalid [B] int32 = first seat whose card is not in its hand or -1 (the
   reference raises InvalidMoveException, env.py:114-118; the game is left
   untouched).  Any output may be NULL.  flags: SN_AUTO_RESET. */
sn_status sn_step(sn_env* env, const int32_t* actions, int32_t* rewards, uint8_t* done, int32_t* invalid, int flags,
                  void* stream);

/* Fused self-play: `steps` env-steps of every game with the DrunkHamster
   policy in one launch (GameSession.play_game, play.py:23-75, looped with
   auto-reset).  Per-step outputs, each optional (NULL):
     rewards [steps][B][N] int32, done [steps][B] uint8,
     actions [steps][B][N] uint8,
     obs     [steps][B][N][obs_stride] int8: the observation each seat acts
             on (env.py:174-212, pre-action), zero-padded to obs_stride >= L.
             obs_stride is a multiple of 4 and obs 4-byte aligned; rows of
             obs_stride == 48 leave as 16-byte pieces, so such an obs must be
             16-byte aligned.  A violation is SN_EINVAL before anything is
             launched or any handle state changes.
   flags: SN_AUTO_RESET (required when steps run past a game's end),
          SN_NO_SUMMARIES. */
sn_status sn_rollout(sn_env* env, int steps, int32_t* rewards, uint8_t* done, uint8_t* actions, int8_t* obs,
                     int obs_stride, int flags, void* stream);

/* env.py:174-212 _create_states: obs [B][N][obs_stride] of `dtype`
   (L = 47, or 35 with SN_NO_SUMMARIES; padding is zero). */
sn_status sn_obs(sn_env* env, void* obs, int dtype, int obs_stride, int flags, void* stream);
/* legal_actions (env.py:209): hands [B][N][10] int8 ascending, -1 padded */
sn_status sn_hands(sn_env* env, int8_t* hands, void* stream);
/* the board (env.py:30,191-194): [B][4][6] int8, -1 padded */
sn_status sn_board(sn_env* env, int8_t* board, void* stream);
/* _scores (env.py:32,167): [B][N] int32 penalties so far this episode */
sn_status sn_scores(sn_env* env, int32_t* scores, void* stream);
/* episode accumulators for auto-reset play (GameSession.results,
   play.py:74): sum over finished episodes of the final scores (-penalty)
   [B][N] int32, and the finished-episode count [B] int32.  Either may be NULL. */
sn_status sn_results(sn_env* env, int32_t* sum_results, int32_t* episodes, void* stream);
sn_status sn_clear_results(sn_env* env, void* stream);

/* numpy global-RNG bridge for the drop-in scalar API [sync]: export /
   import game g's MT19937 state in np.random.get_state() form
   (key_host[624] uint32, pos_host in 0..624). */
sn_status sn_mt_get(sn_env* env, int64_t game, uint32_t* key_host, int32_t* pos_host);
sn_status sn_mt_set(sn_env* env, int64_t game, const uint32_t* key_host, int32_t pos);
/* philox word counter of game g [sync] */
sn_status sn_philox_counter(sn_env* env, int64_t game, uint64_t* counter_host);

/* ---- Whole-handle snapshots (checkpoint / resume, resharding) -------------
   A snapshot is one contiguous blob in DEVICE memory, 16-byte aligned: a
   fixed header (magic, format version, record size; B, N, C, rng_mode, seed,
   game_offset; the league configuration; the host fields phase / lg_phase),
   then one fixed-size record per game, game-major: game g at header_bytes +
   g * record_bytes.  A record holds the game (hands, rows, scores, episode
   sums and count), on tournament handles the seat word and the MCS card
   memory, and the RNG in canonical form: numpy-MT as np.random.get_state()'s
   (pos, key[624]) at the play consumer's position, Philox as its 64-bit word
   counter.  A game that has drawn the last word of a round shows that
   round's key at pos 624, as numpy does (it twists at the next draw), never
   the next round's at pos 0; pos 0 is saved only for a state imported at
   pos 0 and not drawn from since.  Records do not depend on the SN_OPT_* settings or on where the
   pipelines stand (tests/test_gpu_snapshot_states.py: every record against
   numpy's own state and the blobs of eight settings byte for byte, at every
   stream position), so a range of records is the state of a shard
   (csrc/sechs_snapshot.h owns the layout; DESIGN.md has the table of what is
   saved and what the next launch rebuilds).
   sn_state_bytes: header + num_games records, pure host arithmetic (no GPU
   is touched); league != 0: the records of a tournament handle.  -1 for
   arguments out of range.  sn_state_size: the same for a handle as it is
   configured now.
   sn_state_save: behind the pipeline sync, on `stream`; the handle is only
   read (it plays on exactly as without the save).  SN_EINVAL: NULL, a blob
   not 16-byte aligned or smaller than sn_state_size; SN_ERNG: the host
   mirror shows that the handle has counted a pipeline overrun (its streams
   are lost).  The mirror lags the device, and the call does not wait for
   it: the kernel writes the device's count, as it stands behind the
   pipeline sync, into the header, and sn_state_load refuses (SN_EINVAL) a
   blob whose count is not zero.
   sn_state_load [sync]: game g of the handle takes record first + g.  The
   header is read back to the host and checked before anything is launched
   or any handle state changes: magic, version, record size, N, C, rng_mode
   and seed must equal the handle's, the league configuration
   (sn_league_config and sn_league_agents) too, first + B must not pass the
   blob's records, blob_bytes must cover them, and blob.game_offset + first
   must equal the handle's game_offset -- every Philox stream and every
   engine draw is keyed by the global game id.  A mismatch is SN_EINVAL with
   a message and the handle is untouched.  A record's pos above 624 is read
   as 624 (the next draw twists).  After a load the overrun count is
   zero and the next rollout starts its pipeline from the plain state. */
int64_t sn_state_bytes(int64_t num_games, int num_players, int rng_mode, int league, int64_t* header_bytes,
                       int64_t* record_bytes);
int64_t sn_state_size(const sn_env* env);
sn_status sn_state_save(sn_env* env, void* blob, int64_t blob_bytes, void* stream);
sn_status sn_state_load(sn_env* env, const void* blob, int64_t blob_bytes, int64_t first, void* stream);

/* Tuning knobs of the numpy-compat DrunkHamster rollout (results never
   depend on them; the tests run both ways):
     SN_OPT_RING_WORDS   words each game's stream is twisted ahead per
                         launch by k_mt_prep (multiple of 64, 64..512;
                         0 = no ring, k_play twists lazily per lane).
                         Default 256 for N <= 4, else 512.
     SN_OPT_CHUNK_STEPS  env-steps per k_mt_prep-fed launch (>= 1, default 10).
     SN_OPT_PIPELINE     1 (default): DrunkHamster rollouts in numpy mode keep
                         each stream twisted ~600 words ahead with k_mt_ahead
                         on a side stream, concurrently with the previous
                         launch's k_play (N <= 6); 0: the paths above.
     SN_OPT_TIMING       n > 0: record HIP events around the next n
                         pipelined k_play / k_mt_ahead launches, each on the
                         stream it runs on (read with sn_kernel_times);
                         0 (default): off.
     SN_OPT_PIPE_GPW     games per k_play wave on the pipelined path: 64
                         (one per lane) or 32 (half the LDS per wave, two
                         waves per SIMD).
     SN_OPT_PIPE_LEAD    words k_mt_ahead keeps twisted past the consumer
                         (64..600, default 600).  TEST KNOB: below 600 the
                         overrun bound of sn_pipe_errors no longer holds;
                         it exists to exercise the SN_ERNG path.
     SN_OPT_PLAY_SPLIT   role-split k_play (producer waves decode every random
                         decision into LDS beside the play waves) for in-kernel
                         DrunkHamster rollouts of a Philox handle whose games
                         are in lockstep (after sn_reset; N <= 4, auto-reset):
                         1 (default) or 0 (never).  Measured (65 536 x 4p):
                         74 -> 59 us per 10 env-steps.  Numpy-compat handles
                         always use the pipelined one-wave k_play.
     SN_OPT_PLAY_QUAD    removed (round 6): k_play_quad, four lanes per game,
                         measured slower; SN_EUNSUPPORTED.
     SN_OPT_TWIST_ROUND  1 (default): the pipelined twist-ahead k_mt_ahead
                         twists whole MT19937 rounds (each old word read
                         once, each new word written once: 8 instead of 12
                         B of MT-state traffic per word); 0: exactly the
                         words the lead needs.  Same words either way.
     SN_OPT_TWIST_EVERY  K = 1 .. 5 (default 4): play launches in groups of
                         K; one k_mt_ahead beside the first launch of each
                         group twists 600 K words past the consumer (the
                         next 2K launches' draws), and that launch waits for
                         the twist of the group before only -- per group one
                         cross-stream wait and one record instead of one per
                         launch.
     SN_OPT_PIPE_FUSED   removed (round 6): the twist folded into k_play_quad,
                         measured slower; SN_EUNSUPPORTED.
     SN_OPT_PIPE_DEC     1 (default): pipelined numpy-compat DrunkHamster rollouts
                         with auto-reset of a plain handle of N <= 4 whose games
                         are in lockstep (after sn_reset) decode ahead: on a
                         second side stream, concurrent with each group's
                         twist (reading the words the twist before produced),
                         k_decode walks every game's ring a group ahead of the
                         play launches and writes one record per episode
                         (its draws, the next deal's sorted hands and rows, the
                         stream offsets), and k_play plays from the records
                         with no RNG work; 0: k_play draws from the ring itself.
                         Same words, same outputs, same exported numpy states.
     SN_OPT_TWIST_SKIP   TEST KNOB: 1 = every steady twist after the first
                         group's twists nothing, so the default schedule
                         runs its ring dry (the SN_ERNG / sn_pipe_errors
                         path); 0 (default): off.
     SN_OPT_TWIST_DEPTH  0 .. 3 (default 3): refill hysteresis of the whole-round
                         twist-ahead (SN_OPT_TWIST_ROUND 1).  A game whose
                         lead is at least the low threshold (600 K words,
                         600 (K + 1) with decode-ahead) twists nothing in a
                         k_mt_ahead dispatch; one below it twists whole rounds
                         until the lead reaches the threshold + 624 depth.
                         The rounds of a refill are chained in LDS, so the
                         2 496-byte MT state is read and written once per
                         refill instead of once per round, and the start-up
                         twist staggers the games (+ 624 (game mod (depth +
                         1)) words) so that they refill in different
                         dispatches.  0 keeps the plain thresholds.  Same
                         words, same outputs, same exported numpy states;
                         the environment variable SECHS_TWIST_DEPTH
                         overrides the default at sn_create.
     SN_OPT_PLAY_GROUP   1 (default): a decode-ahead rollout of more than one
                         chunk (SN_OPT_CHUNK_STEPS) plays its consecutive
                         chunks of one twist group (SN_OPT_TWIST_EVERY = K, so
                         up to K chunks, never across a group boundary) in one
                         k_play launch, which moves from episode record to
                         episode record at every deal; the twists, decodes and
                         the waits between groups stay where they are.  0: one
                         launch per chunk.  Tournament handles and the
                         ring-reading paths keep one launch per chunk (their
                         launches are bounded by the ring window).  Same
                         outputs, same exported numpy states.
     SN_OPT_DEC_WALK     1 (default): k_decode reads the DrunkHamster draws of a
                         step straight from its LDS window by stream position,
                         16 words per look, as it reads the shuffle targets;
                         a step with fewer than 16 live window bytes left (a
                         short lead, an overrun) goes through the byte buffer.
                         0: every step's draws go through the byte buffer (the
                         form before round 10).  Read at every k_decode
                         dispatch.  Same records word for word, so the same
                         outputs and exported numpy states; the environment
                         variable SECHS_DEC_WALK overrides the default at
                         sn_create.
     SN_OPT_DEC_EARLY    1 (default): k_decode touches the next episode's ring
                         window -- one dword of each 64-byte ring chunk it
                         spans, five at most -- as soon as the window's
                         position is known, behind the swap targets, so the
                         window's own loads at the top of the next episode
                         find their lines in L2.  The touched bytes are
                         dropped: they feed nothing and count no overrun, and
                         the last episode of a dispatch touches nothing.
                         0: no touches (the form before round 11).  Read at
                         every k_decode dispatch.  Same records word for
                         word; the environment variable SECHS_DEC_EARLY
                         overrides the default at sn_create.
   A pipelined (numpy-compat) rollout records its ordering event on the
   caller's stream before it returns; every later call waits on that event
   (also on the same stream), so the caller may destroy the stream after
   the call. */
enum { SN_OPT_RING_WORDS = 1, SN_OPT_CHUNK_STEPS = 2, SN_OPT_PIPELINE = 3, SN_OPT_TIMING = 4, SN_OPT_PIPE_GPW = 5,
       SN_OPT_PIPE_LEAD = 6, SN_OPT_PLAY_SPLIT = 7, SN_OPT_PLAY_QUAD = 8, SN_OPT_TWIST_ROUND = 9,
       SN_OPT_TWIST_EVERY = 10, SN_OPT_PIPE_FUSED = 11, SN_OPT_TWIST_SKIP = 12, SN_OPT_PIPE_DEC = 13,
       SN_OPT_TWIST_DEPTH = 14, SN_OPT_PLAY_GROUP = 15, SN_OPT_DEC_WALK = 16, SN_OPT_DEC_EARLY = 17 };
sn_status sn_set_option(sn_env* env, int option, int value);
/* pipelined rollouts whose draws ran past the twisted words (must be 0; a
   nonzero count means those games' draws are wrong) [sync].  The count is
   also mirrored asynchronously into pinned host memory after every
   pipelined rollout: sn_rollout returns SN_ERNG once a completed rollout
   has counted one (sticky for the handle). */
sn_status sn_pipe_errors(sn_env* env, uint32_t* count);
/* mean launch duration (ms) of the pipelined k_play and k_mt_ahead launches
   recorded since SN_OPT_TIMING was set; *n = launches recorded [sync] */
sn_status sn_kernel_times(sn_env* env, float* play_ms, float* ahead_ms, int32_t* n);
/* the same, and the mean duration of the k_decode launches (decode-ahead
   mode; 0 if none ran) [sync] */
sn_status sn_kernel_times_dec(sn_env* env, float* play_ms, float* ahead_ms, float* decode_ms, int32_t* n);
/* Diagnostics (no reference counterpart): shader-clock cycles every k_play
   wave spent per phase of its step loop since the last call, summed over
   waves -- out[0..10] = prologue, obs, draws, resolve, output stores, deck
   shuffle targets, epilogue, hand sorting, deck shuffle swaps, and (role-
   split play waves) the waits at the two barriers; out[11..18] = the split
   kernel's producer waves: draws, barrier 1, shuffle targets, swaps, hands,
   later draws, barrier 2, state store, twist-ahead; out[20] = play waves,
   out[21] = producer waves.  Only the libsechs_prof.so build
   (-DSECHS_PHASE_PROF) records them; the product build returns
   SN_EUNSUPPORTED [sync]. */
sn_status sn_debug_phases(uint64_t* out, int n);
/* k_puct_rollouts phase counters of a -DSECHS_PHASE_PROF build (diagnostics):
   out[0..4] = shader-clock cycles summed over waves in the state copy-in, the
   seat rows, the per-seat layer-1 MFMA, the candidate tiles and the step;
   out[7] = waves; read and cleared.  SN_EUNSUPPORTED in the product library. */
sn_status sn_debug_puct_phases(uint64_t* out, int n);
/* pipeline words to the host (tests, diagnostics) [sync]: what 0 = pabsc[slot]
   (consumer positions, slots 8 and 9 = the decoder's two; B words), 1 =
   ptend[slot] (B words), 2 = decode-ahead record slot (kDecQuads x B 16-B
   pieces, piece-major), 3 = the MT19937 state codes mt_pos[g] as they stand
   (slot 0; B words: twist pointer | twisted-unconsumed words << 16, the form
   a pipeline sync leaves -- read it right after a call that synchronises the
   pipelines, such as sn_state_save, to see which conversion each game's
   record went through).  No pipeline state is changed. */
sn_status sn_debug_pipe_words(sn_env* env, int what, int slot, uint32_t* out);
/* Device-side invariant checks (SN_DASSERT in sechs_env.hip and its headers:
   a played card is in its seat's hand, the cards of a step are distinct, a
   card goes to a row ending below it (or undercuts), rows hold 1..5 cards,
   a deal gives ten distinct cards per hand): violations counted since the
   last call, *first_line = the smallest source line that failed; the
   counters are cleared.  selftest != 0 first runs one deliberately failing
   check.  Only the libsechs_debug.so build (-DSECHS_DEBUG) has them; the
   product build returns SN_EUNSUPPORTED [sync]. */
sn_status sn_debug_failures(uint32_t* count, uint32_t* first_line, int selftest);

/* ---- One-game fast path (the scalar drop-in SechsNimmtEnv) ------------
   For a handle of B == 1: one kernel launch and one stream sync per call
   (host-memory arguments and results; pinned, device-mapped buffer inside
   the handle).  out_host: int32 [2 + 15N] = first illegal seat or -1
   (env.py:114-118; nothing changes then), done, rewards [N] (env.py:64-77),
   scores [N] (penalties so far), then the N observation rows as int8 bytes,
   48 per seat (47 used, env.py:174-212), then per seat the placement of its
   card for the debug trace (env.py:128,145,165): target row | undercut
   (_pick_row_to_replace) << 2 | scored (_score_row) << 3 | penalty << 8
   (all 0 after an illegal step or a reset). [sync] */
sn_status sn_step1(sn_env* env, const int32_t* actions_host, int32_t* out_host, int flags);
/* env.py:43-51 reset() drawing from the numpy legacy state (key, pos) given
   -- np.random.get_state() -- and returning the advanced state for
   np.random.set_state(); out_host as sn_step1 (invalid -1, rewards 0).
   numpy-compat handles only. [sync] */
sn_status sn_reset1(sn_env* env, const uint32_t* key_host, int32_t pos, uint32_t* key_out_host, int32_t* pos_out,
                    int32_t* out_host, int flags);

/* ---- Batched tournament (tournament.py:132-177) ------------------------
   A tournament handle plays one league game per game slot at a time: slot
   g is the reference's `np.random.seed(seed + game_offset + g); t =
   Tournament(min_players, max_players) over num_agents DrunkHamster
   agents; t.play_game() x games` -- every game first draws its seats
   (_choose_players: num_players = choice(range(min, max+1)), agents =
   choice(num_agents, num_players, replace=False)), then GameSession deals
   and plays it, all from the slot's own stream.  The handle's num_players
   is max_players; seats past a game's player count hold empty hands and
   play nothing.  In-kernel DrunkHamster seats only (the search agents play
   through the drop-in Tournament).  Elo (order dependent) is replayed on
   the host from the records (sn_elo_replay). */
/* turn a handle (num_players = max_players, 2..6) into a tournament of
   num_agents (max_players..16) agents; 0 agents turns it back.  The next
   sn_reset draws every slot's first seats and deals [sync]. */
sn_status sn_league_config(sn_env* env, int num_agents, int min_players, int max_players);
/* play steps/10 whole games per slot (auto-reset: each finished game's
   slot draws its next seats and deals).  records: [steps/10][B][1 + N]
   int32 per finished game: seats word (k | agent(seat p) << (4 + 4p)),
   then the N results (GameSession.results[0]: -penalties; 0 past k).
   rewards/done/actions/obs as sn_rollout (may be NULL). */
sn_status sn_league_rollout(sn_env* env, int steps, int32_t* rewards, uint8_t* done, uint8_t* actions, int8_t* obs,
                            int obs_stride, int32_t* records, void* stream);
/* the seats word of every slot's current game, [B] uint32 */
sn_status sn_league_seats(sn_env* env, uint32_t* out, void* stream);

/* Mixed leagues (run.py:20-40: DrunkHamster, MCSAgent, PUCTAgent,
   PUCTCustomedAgent, BatchedACERAgent seats).  sn_league_agents gives every
   agent of a tournament handle its kind (kinds[num_agents]; all
   SN_AGENT_RANDOM after sn_league_config):
     SN_AGENT_RANDOM    DrunkHamster, drawn in-kernel from the slot's stream
     SN_AGENT_MCS       MCSAgent(mc_per_card[a], mc_max[a]) (agents/mcts.py:17-188):
                        the card memory and the search.  numpy handles: the
                        reference-exact search on the slot's stream.  Philox
                        handles: one stream per playout, by the stream law at
                        sn_league_step -- the reference's search in law, not
                        draw for draw; mc_max[a] > 1 << 20 is SN_EINVAL
                        there (a playout's number is a 20-bit field of its
                        stream word)
     SN_AGENT_EXTERNAL  the caller plays the seat (the net agents: their
                        batched engines pick the card, sn_puct over the
                        handle's decision list, sn_puct.dec_list)
   mc_per_card / mc_max may be NULL (10 / 100, mcts.py:24-25).  Leagues with
   any non-RANDOM agent play with sn_league_step; all-RANDOM ones also with
   sn_league_rollout. [sync] */
enum { SN_AGENT_RANDOM = 0, SN_AGENT_MCS = 1, SN_AGENT_EXTERNAL = 2 };
sn_status sn_league_agents(sn_env* env, const int32_t* kinds_host, const int32_t* mc_per_card_host,
                           const int32_t* mc_max_host);
/* One env-step of every slot's current game (sn_reset then 10 steps per
   game): seats in seat order as GameSession calls
   them (play.py:38-41) -- on a numpy handle RANDOM and MCS seats draw from
   the slot's stream in the reference's exact order, on a Philox handle by
   the stream law below; EXTERNAL seats play actions [B][N] (checked
   against the hand, env.py:114-118).  A game that ends (every 10th step)
   writes records [B][1 + N] (seats word, GameSession.results[0]); the
   slots' next games start with sn_reset (seat draw, then deal:
   tournament.py:132-138), after any roster change.  Outputs (each may
   be NULL): rewards [B][N], played [B][N] (cards, -1 past k), invalid [B]
   (first seat whose external card is illegal, or -1: that slot's board,
   hands and scores are left as they were, but its RANDOM / MCS seats have
   already drawn this step from the slot's stream and an MCS seat's card
   memory has moved on -- the slot no longer follows the reference's stream
   and the caller must treat it as failed; the batched tournament raises right
   after such a step), status [B] |= 1 where an MCSAgent move got no playout
   (the reference raises IndexError there, quirk Q6).

   The stream law of a Philox tournament handle (rng_mode SN_RNG_PHILOX,
   seed = seed_hi << 32 | seed_lo; slot g, gid = game_offset + g).
   Main stream: key (seed_lo, seed_hi), stream gid, word counter ctr[g]
   (sn_philox_counter).  sn_reset draws the seats, then the deal.  In
   sn_league_step the RANDOM seats draw legal[random_interval(n - 1)] from
   it in seat order; EXTERNAL and MCS seats draw nothing from it.  (An
   illegal external card leaves the slot's counter where it was.)
   MCS decision of seat p at a hand of n >= 2 cards in a game of k players,
   c0 = ctr[g] as the step begins, before any RANDOM seat of the step draws:
   playout j, 0 <= j < n_mc = min(mc_max, mc_per_card * n!), draws from a
   Philox stream of its own, from word 0:
     key     (seed_lo ^ lo32(c0), seed_hi ^ hi32(c0) ^ 0x4D435331)
     stream  (uint32)gid << 32 | p << 28 | j << 8 | n
   (the layout of the net engines' decision streams: j where a rollout number
   sits, n in the low byte).  Within a game n differs from step to step, and
   between two games sn_reset draws at least the deal, so (c0, n) never
   repeats for a (gid, p).  None of this is state: a snapshot taken
   mid-round resumes the same searches.
   A playout draws in the order of the reference's loop body (mcts.py:108-154
   with uniform moves): from the ascending card memory of A cards, numpy's
   shuffle (i = A-1 .. 1: j = random_interval(i), swap); opponent q = 1 ..
   k-1 holds sorted(cards[(q-1) n : q n]); for t < n and seat q = 0 .. k-1
   idx = random_interval(n - t - 1), seat 0's first idx is the move the
   playout is filed under; outcome = -(seat 0's penalties).
   The move is _choose_action_from_outcomes': the best mean in legal order,
   strict '>', over integer sums and counts (so it does not depend on which
   lane ran which playout); a legal move without a playout sets status bit 1
   and the best sampled move is played (quirk Q6).  A one-card hand is
   played without a search. */
sn_status sn_league_step(sn_env* env, const int32_t* actions, int32_t* rewards, int32_t* played, int32_t* records,
                         int32_t* invalid, int32_t* status, void* stream);
/* Sequential multiplayer Elo over game records in the given order (host
   memory, no GPU): records [G][1 + max_players] int32 as sn_league_rollout
   writes them; elos [num_agents] float64 in/out (initial ratings in).
   Places are Tournament._compute_absolute_positions of the k results,
   ratings update by the multiplayer Elo of rl_6_nimmt/elo.py (multi_elo's
   scheme; parity unpinned: multi_elo is absent). */
sn_status sn_elo_replay(const int32_t* records_host, int64_t num_games, int max_players, int num_agents, double elo_k,
                        double* elos_host);

/* ---- Monte-Carlo search, MCSAgent (agents/mcts.py:17-188) ------------- */

/* Card memory of every seat (mcts.py:62-73), updated in place from the
   current position: at a hand of 10 it restarts as range(mcs_num_cards),
   then the own hand and every card on the board are removed.
   avail: [4][B*N] uint32 card sets (word-major, decision d = g*N + p). */
sn_status sn_mcs_memorize(sn_env* env, uint32_t* avail, int mcs_num_cards, void* stream);

/* Stratified Monte-Carlo search for every (game, seat) at once (BASELINE
   config 3): `rollouts` playouts per legal first move, opponents dealt from
   the seat's memory, every later move uniform (mcts.py:108-154).
   sums [B*N][10] int32 = summed return of the seat per first move (slots
   >= the hand size are 0).  Random words: Philox keyed (seed ^
   decision_step, game id, seat, move, playout).  rollouts: 64, 128, 192 or
   a multiple of 256. */
sn_status sn_mcs_rollouts(sn_env* env, const uint32_t* avail, int rollouts, uint64_t seed, uint32_t decision_step,
                          int32_t* sums, void* stream);
/* same, also writing every playout's return: playouts [B*N][10][rollouts] int32 (may be NULL) */
sn_status sn_mcs_rollouts_ex(sn_env* env, const uint32_t* avail, int rollouts, uint64_t seed, uint32_t decision_step,
                             int32_t* sums, int32_t* playouts, void* stream);

/* _choose_action_from_outcomes (mcts.py:156-165) with equal playout counts:
   actions [B][N] int32 = legal[argmax sums] (ties -> lowest card), legal[0]
   for a one-card hand, -1 for an empty hand. */
sn_status sn_mcs_choose(sn_env* env, const int32_t* sums, int32_t* actions, void* stream);

/* Reference-exact replay (numpy-MT env only): every game of the handle plays
   one whole GameSession game (reset + 10 steps) with seat p an
   MCSAgent(mc_per_card, mc_max) if bit p of mcs_seats is set, else a
   DrunkHamster, consuming the game's MT19937 stream in the reference's
   exact order.  actions / rewards [10][B][N] int32; status [B] = 1 where the
   reference would have raised IndexError (quirk Q6, a move without playouts). */
sn_status sn_mcs_play_exact(sn_env* env, uint32_t mcs_seats, int mc_per_card, int mc_max, int32_t* actions,
                            int32_t* rewards, int32_t* status, void* stream);

/* Reference-exact MCSAgent._mcts for D independent decisions (one wave
   each), for the drop-in agent; num_players K in 1..10.  Device buffers:
   board [D][4][6] int8 (-1 pad), hand [D][10] int8 (the legal actions, -1
   pad), avail [D][4] uint32 card memory, mt_keys [D][624] + mt_pos [D]:
   numpy-form MT19937 states (np.random.get_state()[1:3]) advanced in place.
   actions [D] int32: the chosen card, or -(card)-2 when quirk Q6 applies;
   sums / counts [D][10] (optional) = per-move playout sums and counts.
   A hand of one card is played without a search: sums / counts 0, the state
   untouched.
   Preconditions per decision, on the caller's buffers: a hand of n >= 1
   cards; for n >= 2 a card memory of A cards with max(2, (K - 1) n) <= A <=
   104 (every playout deals the K - 1 opponents n cards each from it); 0 <=
   mt_pos.  A decision that breaks one gets actions[d] = -1, zeroed sums /
   counts, and its (key, pos) left as they were (the reference raises there:
   np.random.choice on an empty hand); the other decisions of the launch are
   not affected. */
sn_status sn_mcs_decide_exact(int device, int64_t num_decisions, int num_players, const int8_t* board,
                              const int8_t* hand, const uint32_t* avail, int mc_per_card, int mc_max,
                              uint32_t* mt_keys, int32_t* mt_pos, int32_t* actions, int32_t* sums, int32_t* counts,
                              void* stream);

/* The Philox league search (the stream law at sn_league_step) for D
   independent decisions, one wave each: the device function the league's
   search kernel runs, for tests.  num_players K in 2..6; board, hand, avail,
   actions, sums, counts as sn_mcs_decide_exact; keys [D][2] uint32 = a
   decision's Philox key, streams [D] uint64 = its stream word with j = 0
   (playout j draws from streams[d] | j << 8); mc_max <= 1 << 20.
   actions[d] = the card, -(card)-2 under quirk Q6, the card of a one-card
   hand (no search, sums / counts 0), or -1 with zeroed sums / counts where
   the hand is empty or the memory does not hold (K - 1) n <= A <= 104 cards;
   the other decisions of the launch are not affected. */
sn_status sn_mcs_decide_philox(int device, int64_t num_decisions, int num_players, const int8_t* board,
                               const int8_t* hand, const uint32_t* avail, int mc_per_card, int mc_max,
                               const uint32_t* keys, const uint64_t* streams, int32_t* actions, int32_t* sums,
                               int32_t* counts, void* stream);

/* ---- "Alpha0.5" PUCT search, PUCTAgent / PolicyMCSAgent (mcts.py:191-323) ----
   The rollouts of one decision are a dependent chain (each root choice reads
   the outcomes so far), so a batch advances rollout `rollout` of every
   decision by one step per call; the policy MLP runs between the calls in
   PyTorch-ROCm.  Per decision d (game g = d / M, seat = the (d % M)-th set
   bit of seats_mask, M = popcount):
     sn_puct_root_rows  rows [D*n][48] (bf16 or f32): [legal[k], obs] normalised
                        as SechsNimmtStateNormalization (preprocessing.py:12-57)
     sn_puct_init       root_probs = softmax(root logits [D*n] f32); clears stats
     for rollout r:  sn_puct_deal (opponents from the memory, mcts.py:116-127)
       for t < n:    sn_puct_rows (rows [D*N*(n-t)][48] of every rollout seat),
                     MLP -> logits [D*N*(n-t)] f32, sn_puct_step (PUCT at the
                     root / policy samples elsewhere, env step, backup at the end)
     sn_puct_choose     actions [B][N] int32 of the deciding seats = best mean
   Buffers (device, caller-owned): rollouts [D][48] i32, stats [D][24] i32,
   hist [D][172] i32, root_probs [D][10] f32.
   The five search buffers (avail, rollouts, stats, hist, root_probs) are
   required by exactly the calls whose kernels read or write them, and those
   calls return SN_EINVAL, naming the field and launching nothing, when one
   they need is NULL:
     sn_puct_init        stats, hist, root_probs
     sn_puct_deal        avail, rollouts        sn_puct_deal_batch  avail
     sn_puct_rows        rollouts               sn_puct_mlp_seats   rollouts
     sn_puct_step        rollouts, stats, hist, root_probs
     sn_puct_rollouts    stats, hist, root_probs
     sn_puct_choose      stats (n > 1)
   They may all be NULL for sn_puct_root_rows, sn_pcv_choose,
   sn_policy_sample and sn_dqn_* (those kernels take only the deciding seats,
   n, seed and step from this struct).
   A rollout number is the 20-bit tag of its Philox streams, and the tags from
   0xFFF00 up belong to the draws outside a rollout (SN_NOISY_TAG, the
   epsilon-greedy draws, the policy sample): sn_puct_deal and sn_puct_step
   (`rollout`), sn_puct_deal_batch and sn_puct_rollouts (r0 + nr - 1) return
   SN_EINVAL and launch nothing when a rollout number reaches 0xFFF00. */
typedef struct {
    uint32_t seats_mask;   /* deciding seats (bit p = seat p) */
    int n;                 /* hand size at the root (all games in lockstep) */
    int puct_root;         /* 1: PUCTAgent (PUCT at the root), 0: PolicyMCSAgent (sampled root) */
    double c_puct;         /* mcts.py:267, default 2.0 */
    uint64_t seed;
    uint32_t step;         /* decision counter, mixed into the Philox key */
    uint32_t rollout;      /* rollout index r */
    const uint32_t* avail; /* [4][B*N] card memory from sn_mcs_memorize */
    int32_t* rollouts;
    int32_t* stats;
    int32_t* hist;
    float* root_probs;
    const uint32_t* step_dev; /* NULL, or the decision counter in device memory (overrides `step`):
                                 lets one captured hipGraph of a decision's launches serve every decision */
    const int32_t* dec_list;  /* NULL (seats_mask), or num_dec decisions g * N + p in device memory: one
                                 agent's seats of a tournament handle (required there); a game of k < N
                                 players then rolls out k seats (obs N field k, mcts.py:62-64) and writes
                                 dummy rows for the absent seats */
    int64_t num_dec;
    int32_t logit_stride;     /* sn_puct_step: elements between consecutive candidates' logits (0 or 1: packed) */
    int32_t logit_bf16;       /* sn_puct_step: the logits are bf16 (e.g. a head GEMM padded to 16 outputs,
                                 logit_stride 16), not f32 */
} sn_puct;

sn_status sn_puct_root_rows(sn_env* env, const sn_puct* q, void* rows, int bf16, void* stream);
sn_status sn_puct_init(sn_env* env, const sn_puct* q, const float* root_logits, void* stream);
sn_status sn_puct_deal(sn_env* env, const sn_puct* q, void* stream);
/* sn_puct_deal for rollouts r0 .. r0 + nr - 1 in one launch: rollout r's
   initial state at ro_out + ((r - r0) * num_decisions + d) * 48 int32 (the
   layout of sn_puct.rollouts); point sn_puct.rollouts at rollout r's slice
   and run its steps there -- the same states, dealt with nr x D lanes. */
sn_status sn_puct_deal_batch(sn_env* env, const sn_puct* q, int r0, int nr, void* ro_out, void* stream);
/* Rollouts r0 .. r0 + nr - 1 of every decision in one launch, from the
   states sn_puct_deal_batch dealt into ro_base: one wave per group of up to
   32 / L decisions (L = N rounded up to 4 or 8; the library picks the
   smallest group that keeps the launch's rounds over its waves at their
   minimum) runs every step (sn_puct_mlp_seats' rows, MFMA layer 1 + 2 and
   head into logits in LDS, then sn_puct_step's seat-lane step) of each
   rollout in order -- the same values as the launch-per-step loop (3 <= N
   <= 8; weights as sn_puct_mlp_seats).  The environment variable
   SECHS_PUCT_GROUP=k forces k decisions per group (clamped to 1 .. 32 / L),
   read at every call: the same values at any group size (A/B runs, tests).
   Its siblings: SECHS_PUCT_STEP_SEATS=0 (sn_puct_step runs the one-lane-per-
   decision kernel at N <= 8 too), and in the Python engine
   SECHS_PUCT_DEAL_BATCH / SECHS_PUCT_ROLLOUTS (puct.py). */
sn_status sn_puct_rollouts(sn_env* env, const sn_puct* q, int r0, int nr, void* ro_base, const void* w1s,
                           const float* w1c, const void* w2, const float* head, void* stream);
sn_status sn_puct_rows(sn_env* env, const sn_puct* q, int n_cur, void* rows, int bf16, void* stream);
sn_status sn_puct_step(sn_env* env, const sn_puct* q, const float* logits, int t, int n_cur, void* stream);
/* Rollout MLP in one kernel per rollout step, for MultiHeadedMLP(48, (H, H2),
   (1,)) in bf16, H <= 111, H2 <= 127 -- the reference's policy net,
   utils/nets.py:100-132, evaluated in mcts.py:219-228: persistent
   workgroups loop over groups of 64 rollout seats, build their [0, obs, 1]
   rows in LDS (the card slot 0), multiply them by w1s [128][64] bf16 (the
   [W1 | b1 | 0] rows, 1 at (H, 48): the ones feature) on MFMA into base,
   then per candidate row h1[k] = bf16(relu(base[seat][k] + card * w1c[k]))
   (w1c = W1[:, 0] f32, 112 entries), layer 2 against w2 [128][112] bf16 =
   [W2 | b2 | 0] rows (+ the ones pass-through row H2), ReLU + bf16, and the
   head [128] f32 = [wh | bh | 0]: logits [D*N*n_cur] f32, packed, for
   sn_puct_step (logit_stride 1, logit_bf16 0).  No activation reaches HBM.
   w1s, w1c, w2, head 16-B aligned.  (The round-4 GEMM form -- seat rows, a
   PyTorch GEMM, a tile kernel -- the round-3 feature-major split and the
   round-5 per-candidate MFMA layer 1 measured slower and were removed in
   round 6; other nets take sn_puct_rows + the module's own forward.) */
sn_status sn_puct_mlp_seats(sn_env* env, const sn_puct* q, int n_cur, const void* w1s, const float* w1c, const void* w2,
                            const float* head, float* logits, void* stream);
/* best_index [D] (optional): index of the chosen card in the root legal list */
sn_status sn_puct_choose(sn_env* env, const sn_puct* q, int32_t* actions, int32_t* best_index, void* stream);
/* PUCTCustomedAgent (agents/mcts.py:325-451, replaces _mcts /
   _play_out_with_NN / _choose_action_mc_func :356-395): no rollouts.  heads
   [D*n][2] f32 = the 2-head net (policy logit, value) on the
   sn_puct_root_rows rows; per decision: best = first argmax of the values,
   actions [B][N] (deciding seats) = legal[best], best_index [D],
   log_prob [D] = log softmax(policy)[best], value [D] = values[best] (the
   "outcome" learn() regresses).  Optional outputs may be NULL. */
sn_status sn_pcv_choose(sn_env* env, const sn_puct* q, const float* heads, int32_t* actions, int32_t* best_index,
                        float* log_prob, float* value, void* stream);
/* BatchedReinforceAgent.forward (agents/policy.py:137-156) for every
   deciding seat of q->seats_mask at hand size q->n: logits [D*n] f32 = the
   policy MLP on the sn_puct_root_rows rows; samples Categorical(softmax)
   with Philox (key q->seed ^ q->step; torch's CPU generator is not
   reproducible on the device), actions [B][N] (deciding seats) = legal[k],
   index [D] = k, log_prob [D], entropy [D] (optional, may be NULL). */
sn_status sn_policy_sample(sn_env* env, const sn_puct* q, const float* logits, int32_t* actions, int32_t* index,
                           float* log_prob, float* entropy, void* stream);
/* _compute_pucts + argmax (mcts.py:282-315) for D given states: n [D],
   stats [D][24] (sums[10], counts[10], total, min, max), hist [D][172]
   outcome counts (value v at bin v+171), probs [D][10] f32 -> pucts [D][10]
   f64, choice [D] (formula test hook). */
sn_status sn_puct_score(int64_t num, const int32_t* n, const int32_t* stats, const int32_t* hist, const float* probs,
                        double c_puct, double* pucts, int32_t* choice, void* stream);

/* ---- Prioritised experience replay (utils/replay_buffer.py:15-203) ------
   The SumTree + PriorityReplayBuffer of the DQN family on the device.  An
   sn_per handle owns a sum tree of 2*capacity-1 f64 nodes in the reference's
   implicit-heap layout for every capacity (root 0, children of i at 2i+1 and
   2i+2, leaves at capacity-1 .. 2*capacity-2, data slot = leaf - capacity + 1:
   the tree indices sample returns go back into update, so the layout is part
   of the interface) and an optional payload ring [capacity][row_bytes].
   After store and update every internal node is left + right, recomputed
   pairwise from the leaves (the reference adds `change` along one path,
   replay_buffer.py:16-27: equal up to its rounding drift).  The pointer and
   the item counter live on the host and move when a call is enqueued, so no
   call synchronises; calls of one handle belong on one stream.
   Two reference quirks are kept (replay_buffer.py:81-104,160-166):
     - num_items grows on every store that does not wrap the pointer, also
       after the buffer is full: len = stores - wraps, past the capacity
       (capacity 5: 35 after 43 stores);
     - min_leaf, the normaliser of the importance weights, is the minimum
       over leaves [0, min(num_items, capacity)): right after the first wrap
       the last leaf is left out. */
typedef struct sn_per sn_per; /* opaque */
/* capacity >= 2 (the reference cannot sample from a one-slot buffer);
   row_bytes 0 (no payload) or a multiple of 16 */
sn_status sn_per_create(sn_per** out, int64_t capacity, int64_t row_bytes, int device);
sn_status sn_per_destroy(sn_per* per);
/* the host counters: SumTree.capacity, .data_pointer, .num_items (each may be NULL) */
sn_status sn_per_info(const sn_per* per, int64_t* capacity, int64_t* pointer, int64_t* num_items);
/* m sequential PriorityReplayBuffer.store calls (replay_buffer.py:150-158),
   1 <= m <= capacity: slots pointer .. pointer+m-1 modulo capacity get the
   priority M = the maximum over all leaves before the call, or 1.0 if that
   is 0 (writing M never changes the maximum, so M is the same for the whole
   batch, as in the reference's loop).  rows: [m][row_bytes] payload copied
   into the same slots (16-byte aligned), or NULL. */
sn_status sn_per_store(sn_per* per, int64_t m, const void* rows, void* stream);
/* PriorityReplayBuffer.sample(n) (replay_buffer.py:160-186) with the caller's
   uniforms u [n] f64 in [0,1): sample i descends with v = seg*i + u[i]*seg,
   seg = total/n (`v <= left` goes left, else subtract and go right,
   :43-60), in the reference's operation order without FP contraction.
   tree_idx [n] uint32; priority [n] f64 = the leaf; is_weight [n] f64 =
   ((p/total)/min_prob)^-beta, min_prob = min_leaf/total; rows_out
   [n][row_bytes] = the payload rows of the sampled slots.  priority,
   is_weight and rows_out may be NULL.  An empty replay is SN_EINVAL (the
   reference's np.min raises). */
sn_status sn_per_sample(sn_per* per, int64_t n, const double* u, double beta, uint32_t* tree_idx, double* priority,
                        double* is_weight, void* rows_out, void* stream);
/* PriorityReplayBuffer.batch_update (replay_buffer.py:188-200): leaf
   tree_idx[i] = min(abs_err[i] + eps, upper)^alpha.  Where an index repeats
   the highest position wins (the reference's sequential loop); indices
   outside the leaf range are skipped, not written. */
sn_status sn_per_update(sn_per* per, int64_t n, const uint32_t* tree_idx, const double* abs_err, double eps,
                        double upper, double alpha, void* stream);
/* the 2*capacity-1 nodes (tests, cloning) */
sn_status sn_per_tree(sn_per* per, double* tree_out, void* stream);
/* The payload rows of n data slots (slots [n] int32 in device memory, slot =
   leaf - capacity + 1) into rows_out [n][row_bytes], 16-byte aligned: the
   gather of sn_per_sample without the tree walk.  A slot outside
   [0, capacity) yields a zero row.  This is the uniform replay of DQNVanilla /
   DDQNAgent: History.sample (replay_buffer.py:233-234) draws
   random.sample(range(len)), the caller draws the slots. */
sn_status sn_per_gather(sn_per* per, int64_t n, const int32_t* slots, void* rows_out, void* stream);
/* A clone's replay (the reference's copy_player round-trips the whole agent
   through torch.save, tournament.py:54-60: the clone is the same buffer).
   Every slot of dst is overwritten, then its internal nodes are recomputed
   as after store and update.  src is only read; its pending work must have
   been enqueued on `stream` as well (the call only enqueues, like every
   sn_per_* call, and does not wait for another stream).  SN_EINVAL: a NULL
   argument, dst == src, different row_bytes, different devices.
     - Equal capacities: a verbatim copy.  Every leaf and row keeps its slot,
       pointer and num_items are copied (num_items past the capacity too), so
       dst and src answer the same uniforms with the same tree indices.
     - Different capacities: the newest rows are re-homed.  held = src's
       capacity if src has wrapped, else its pointer; src has wrapped exactly
       when num_items != pointer (before the first wrap both count the stores;
       after w wraps num_items - pointer = (capacity - 1) * w >= 1).
       h = min(held, dst's capacity); slot k < h of dst (0 = the
       oldest) takes the leaf -- src's priority, not the maximum -- and the
       row of src's slot (pointer - h + k) mod capacity; slots k >= h get a
       zero leaf and a zero row.  dst's counters become those of h stores
       into an empty ring: pointer = h mod capacity, num_items = h, less one
       if h equals the capacity (that store wrapped). */
sn_status sn_per_inherit(sn_per* dst, const sn_per* src, void* stream);
/* The verbatim copy from caller-owned device buffers (un-pickling; the
   export is sn_per_tree's leaves and sn_per_gather of every slot): leaves
   [capacity] f64, rows [capacity][row_bytes] 16-byte aligned -- NULL exactly
   when row_bytes is 0 --, neither overlapping dst's own memory; pointer in
   [0, capacity), num_items >= 0, else SN_EINVAL. */
sn_status sn_per_import(sn_per* dst, const double* leaves, const void* rows, int64_t pointer, int64_t num_items,
                        void* stream);

/* ---- Batched DQN family (agents/dqn.py:42-231,304-380,427) ---------------
   Every deciding seat of every game acts together; decisions are addressed
   through sn_puct exactly as sn_policy_sample's (seats_mask, or dec_list /
   num_dec, plus n, seed, step).  The Q net, MultiHeadedMLP(47, hidden,
   (104,)), runs between the calls in PyTorch-ROCm.

   sn_dqn_obs: the observation a DQN agent acts on, the raw _create_states row
   (env.py:174-212; GameSession hands it over un-normalised).  obs_i8 [D][48]
   int8 = the 47 values and one zero pad byte (the replay payload form);
   states [D][48] f32 (bf16 = 0) or bf16 (bf16 = 1) = the same values as
   floats, column 47 zero (every value lies in -1..104, so bf16 holds it
   exactly).  Either output may be NULL; both 16-byte aligned.  In a
   tournament game of k < N players field 10 (the player count) is k, as in
   sn_puct_root_rows.  q->n is not used, and 0 is accepted: after a game's
   last step the hand is empty and the row is the terminal next_state. */
sn_status sn_dqn_obs(sn_env* env, const sn_puct* q, void* obs_i8, void* states, int bf16, void* stream);
/* _action_selection (agents/dqn.py:196-217): epsilon-greedy over the hand.
   qvals [D][q_stride] f32, q_stride >= 104: the Q head over all 104 cards.
   Per decision two Philox uniforms u1, u2 keyed like sn_policy_sample's
   (q->seed ^ q->step, game, seat) under a rollout tag of their own.  Greedy
   when u1 > eps: action = legal[k], k the first maximum of Q[legal[j]] over
   the ascending legal list (numpy's first arg-max of the -1e8-masked vector
   for any Q > -1e8), value = Q[action]; else action = legal[floor(u2 * n)],
   value = -1.  eps <= 0 never explores, eps >= 1 always does.  actions
   [B][N] int32 (deciding seats only), index [D] = k, value [D] f32; index
   and value may be NULL. */
sn_status sn_dqn_select(sn_env* env, const sn_puct* q, const float* qvals, int64_t q_stride, double eps,
                        int32_t* actions, int32_t* index, float* value, void* stream);
/* The transitions of one episode as replay rows (the experience dicts of
   DQNVanilla.learn, agents/dqn.py:87-108: state, action, reward, next_state,
   done).  obs_i8 [T+1][D][48] (sn_dqn_obs before every step and after the
   last), actions [T][D] int32 (stored as one byte), rewards_seen [T][D]
   int32 -> rows [T*D][112], t-major then decider:
     bytes 0-47 state = obs[t], 48-95 next_state = obs[t+1], 96 action (card),
     97 done (1 only at t = T-1), 98 hand size at state, 99 zero,
     100-103 reward int32, 104-111 zero.
   obs_i8 and rows 16-byte aligned. */
sn_status sn_dqn_pack(int64_t T, int64_t D, const void* obs_i8, const int32_t* actions, const int32_t* rewards_seen,
                      void* rows, void* stream);
/* the inverse for n sampled rows (_prep_minibatch, agents/dqn.py:143-168):
   states, next_states [n][48] f32, action [n] int64, reward [n] f32,
   not_done [n] f32 = 1 - done.  Each output may be NULL. */
sn_status sn_dqn_unpack(int64_t n, const void* rows, float* states, float* next_states, int64_t* action,
                        float* reward, float* not_done, void* stream);
/* k_dqn_select for a duelling net (DuellingDQNNet, utils/nets.py:135-144) over
   its padded head output, read in place: heads [D][stride] f32 with V in
   column v_col and A in the 104 columns a_off .. a_off + 103 (both inside the
   row, V outside A).  Per decision Q_c = V + (A_c - mean) in fp32, unfused,
   mean = sum / 104.0f, the sum of A over all 104 actions in this order: four
   partial sums s_k over the columns c = k (mod 4), each ascending, then
   (s_0 + s_1) + (s_2 + s_3).  Everything else is sn_dqn_select's: the same
   Philox keys, the first maximum over the ascending hand, value = Q of the
   choice (-1 when exploring), a card byte past the hand ends the scan.  Rows
   whose A starts 16-byte aligned (heads + a_off aligned, stride a multiple of
   4) are read with 16-byte loads, others with 4-byte loads: the same result. */
sn_status sn_dqn_select_duel(sn_env* env, const sn_puct* q, const float* heads, int64_t stride, int64_t v_col,
                             int64_t a_off, double eps, int32_t* actions, int32_t* index, float* value, void* stream);
/* The n-step transitions of one episode (DQN_NStep_Agent._store and
   _finish_episode, agents/dqn.py:264-301), T <= 10 steps, n >= 1 (else
   SN_EINVAL).  Inputs as sn_dqn_pack's; gpow.v[i] = gamma ** i as the host
   computes it (CPython's float power: no device pow takes part).  Row (s, d),
   with m = min(n, T - s):
     bytes 0-47 state = obs[s], 48-95 next_state = obs[min(s + n, T)],
     96 action, 97 done = (s + n > T) or (n == 1 and s == T - 1), 98 hand size,
     99 m, 100-103 r_s int32, 104-107 the n-step return as f32: accumulated in
     f64 from 0.0, left to right, acc = acc + (double)r_{s+i} * gpow.v[i] for
     i < m (unfused), rounded once; 108-111 zero.
   Kept from the reference: for n > 1 the row s = T - n points at the terminal
   observation with done 0. */
#define SN_DQN_T_STEPS 10
typedef struct {
    double v[SN_DQN_T_STEPS];
} sn_dqn_gpow;
sn_status sn_dqn_pack_nstep(int64_t T, int64_t D, int64_t n, sn_dqn_gpow gpow, const void* obs_i8,
                            const int32_t* actions, const int32_t* rewards_seen, void* rows, void* stream);
/* sn_dqn_unpack with reward = the f32 n-step return at byte 104 */
sn_status sn_dqn_unpack_nstep(int64_t n, const void* rows, float* states, float* next_states, int64_t* action,
                              float* reward, float* not_done, void* stream);
/* Both Bellman targets over q_next_local / q_next_target [n][stride] f32
   (stride >= 104; the maximum runs over all 104 actions, unmasked, as in the
   reference).  q_next_target NULL: DQNVanilla._calc_reward
   (agents/dqn.py:182-194) = reward + gamma * (max_a Q_local(s') * not_done);
   else DDQNAgent._calc_reward (agents/dqn.py:323-340) = reward + gamma *
   (Q_target(s')[argmax_a Q_local(s')] * not_done), the lowest index on ties.
   fp32 in exactly that operation order, unfused; gamma is rounded to f32
   once, as torch rounds the Python scalar: bit-equal to the torch fp32
   expression on the same tensors.  The n-step agents pass gamma ** n_steps. */
sn_status sn_dqn_target(int64_t n, const float* q_next_local, const float* q_next_target, int64_t stride,
                        const float* reward, const float* not_done, double gamma, float* target, void* stream);

/* The noisy DQN nets (NoisyFactorizedLinear, utils/nets.py:36-63): factorised
   Gaussian noise of its own for every decision row.  For decision d (game g,
   seat p of the handle, q's deciders in sn_dqn_select's order), linear layer l
   (forward order: the latent layers, then the heads; l < 64) and side s
   (0: the layer's inputs, 1: its outputs):
     tag = SN_NOISY_TAG(l, s) = 0xFFF00 + 2 l + s,
     Philox4x32-10 key (seed_lo ^ step, seed_hi), counter (i, 0, stream lo,
     stream hi) with stream = gid << 32 | p << 28 | tag << 8 and gid =
     game_offset + g; the block's words o give the units 2 i and 2 i + 1:
       u1 = ((o[0] >> 8) + 1) * 2^-24 in (0, 1],  u2 = (o[1] >> 8) * 2^-24,
       r = sqrtf(-2 logf(u1)),  n = r cosf(2 pi u2), r sinf(2 pi u2)
     in fp32 with the accurate library functions (|n| <= sqrt(48 ln 2)), and
     the value used is e = sign(n) sqrt|n|.
   The noise depends on (seed, step, global game, seat, layer, side, unit)
   only.  Every call returns SN_EINVAL for a NULL handle or pointer, width < 1
   or a tag outside SN_NOISY_TAG(0, 0) .. SN_NOISY_TAG(63, 1).  One lane per
   (row, unit pair).
   sn_noisy_eps: out [D][width] f32 = e of the units 0 .. width - 1. */
#define SN_NOISY_TAG(layer, side) (0xFFF00 + 2 * (layer) + (side))
sn_status sn_noisy_eps(sn_env* env, const sn_puct* q, int64_t tag, int64_t width, float* out, void* stream);
/* out[d][k] = x[d][k] * e_k for k < width: the product in fp32, rounded once to
   the dtype of x and out (bf16 != 0: bfloat16, else f32).  Rows of x_stride /
   out_stride elements, both >= width (else SN_EINVAL); x and out lie apart. */
sn_status sn_noisy_scale(sn_env* env, const sn_puct* q, int64_t tag, const void* x, int64_t x_stride, int64_t width,
                         int bf16, void* out, int64_t out_stride, void* stream);
/* Over the columns j = col0 .. col0 + width - 1 of rows of `stride` floats
   (inside the row, else SN_EINVAL): out[d][j] = mu[d][j] + e_{j - col0} *
   (sg[d][j] + sigma_b[j]) in fp32 in that order, every operation rounded (no
   fma): bit-equal to the torch fp32 expression; then max(., 0) if relu.
   sigma_b is indexed by the column j itself.  out may be mu; the other columns
   are left as they are. */
sn_status sn_noisy_combine(sn_env* env, const sn_puct* q, int64_t tag, const float* mu, const float* sg, int64_t stride,
                           int64_t col0, int64_t width, const float* sigma_b, int relu, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
