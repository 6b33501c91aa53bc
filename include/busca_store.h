/*
 * busca_store.h - appearance state that lives on the device, as calls of libbusca_store.so: a third library next to libbusca_hip.so and
 * libbusca_track.so that needs no busca_ctx (no weights, no workspace, no per-context state).  Two tenants:
 *   GHOST's Track features (adapters/GHOST/src/tracking_utils.py:83-89, 286-289, 342-343; tracker.py:252-255): per track slot a ring of the newest
 *   `budget` features and the moving average get_proxy's 'mv_avg' keeps, in device arrays the caller owns,
 *     gallery  f32 [S, budget, E]     count  i32 [S] (samples stored)     newest  i32 [S] (ring row of the newest sample)
 *     mv_avg   f32 [S, E]             mv_seen u8 [S] (the slot has a moving average)
 *   StrongSORT's EMA feature (adapters/StrongSORT/deep_sort/track.py:85-87, 244-248): one smoothed row per target, in row 0 of its slot of
 *     gallery  f32 [S, ring, E]
 * Every call names the slots it serves:  slot  dev i32 [k].  An entry < 0 or >= S is skipped and touches no memory.  The valid slots of one call
 * must be distinct: duplicates race on that slot's state, but every access stays inside the arrays.
 *
 * Conventions of every call:
 *   - returns 0, or a negative code (-1: a refused argument, -2: the HIP runtime reported an error) with a message in busca_store_last_error();
 *   - `device` is made current for the launch and the previous device restored; `stream` is a hipStream_t of that device (NULL: its default stream);
 *   - asynchronous on `stream`; nothing allocates, nothing synchronises; one kernel launch per call;
 *   - every argument is checked before the first HIP call, so a refusal and the empty no-op need no GPU;
 *   - refused with -1: negative sizes or device, budget / ring / E below 1, a NULL required pointer, a float32 or int32 pointer not 4-byte aligned,
 *     and what each call lists;
 *   - float32 arithmetic, every product, sum, quotient and square root rounded once and never contracted to a multiply-add.
 */
#ifndef BUSCA_STORE_H
#define BUSCA_STORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BUSCA_STORE_OK 0
#define BUSCA_STORE_EINVAL (-1)
#define BUSCA_STORE_EHIP (-2)

/* 1000 * major + minor; this header is version 1000. */
int busca_store_version(void);

/* The message of the calling thread's last refused or failed call ("" when there was none).  Thread-local; valid until that thread's next call. */
const char* busca_store_last_error(void);

/* Track.__init__ / add_detection: for i < k, row j = det_index[i] (NULL: j = i) of `feats` becomes the newest sample of s = slot[i].
 *   c = is_new[i] ? 0 : count[s];   mv_seen[s] = 0 where is_new[i];   row = c == 0 ? 0 : (newest[s] + 1) % budget;
 *   gallery[s, row, :] = feats[j, :] (the bits are copied);   newest[s] = row;   count[s] = min(c + 1, budget)
 *   feats  dev f32 [m, E];  det_index  dev i32 [k] or NULL (then k <= m, else refused);  is_new  dev u8 [k] or NULL (no entry starts a new track).
 * A pair whose j is outside 0 .. m-1 is skipped like one whose slot is.  k = 0: returns 0 and launches nothing. */
int busca_store_ring_add(float* gallery, int32_t* count, int32_t* newest, uint8_t* mv_seen, int32_t S, int32_t budget, int32_t E, const int32_t* slot,
                         int32_t k, const float* feats, int32_t m, const int32_t* det_index, const uint8_t* is_new, int32_t device, void* stream);

/* The tracks in the listed slots are gone:  count[s] = 0  and  mv_seen[s] = 0.  k = 0: returns 0 and launches nothing. */
int busca_store_release(int32_t* count, uint8_t* mv_seen, int32_t S, const int32_t* slot, int32_t k, int32_t device, void* stream);

/* get_proxy's 'mv_avg' branch for n listed tracks, the first `num_active` of them with the weight a_act, the others with a_inact:
 *   last = gallery[s, newest[s], :];   f = mv_seen[s] ? mv_avg[s] * wa + last * wb : last,   wa = (float)a, wb = (float)(1.0 - a);
 *   mv_avg[s] = f;   mv_seen[s] = 1;   out[i] = f
 *   count   dev i32 [S] or NULL: every slot holds `budget` samples;  a count is clamped to 0 .. budget
 *   newest  dev i32 [S] or NULL: the newest sample is row count - 1 (also where the entry is outside 0 .. budget-1)
 *   out     dev f32 [n, E], in list order
 * A row whose slot is skipped or holds no sample gets NaN in `out` and leaves the tables untouched.  Bit-exact against torch CPU.
 * Refused: num_active outside 0 .. n, a NaN weight.  n = 0: returns 0 and launches nothing. */
int busca_store_mv_avg(const float* gallery, const int32_t* count, const int32_t* newest, float* mv_avg, uint8_t* mv_seen, int32_t S, int32_t budget,
                       int32_t E, const int32_t* slot, int32_t n, int32_t num_active, double a_act, double a_inact, float* out, int32_t device,
                       void* stream);

/* StrongSORT's smoothed feature for g targets in one launch.  Target i owns slot group_slot[i] and is fed, in this order, the rows
 * src[group_start[i]] .. src[group_start[i + 1] - 1] of `feats`:
 *   feature = f / ||f||;   with a sample (group_old_row[i] >= 0: ring row of the one it has; always after its first feature of this call)
 *   smooth = (float)alpha * old + (float)(1.0 - alpha) * feature,  smooth /= ||smooth||;   without one the target stores `feature`.
 * The result is written to ring row 0 of the slot; what lies between stays on chip.  ||.|| = sqrt of the sum of squares, the sum taken in a fixed
 * order in float64 and rounded once to float32, sqrt and / correctly rounded float32: the same bits every run and whatever g is.  A zero row gives
 * NaN (0 / 0).
 *   feats  dev f32 [m, E];  group_slot, group_old_row  dev i32 [g];  group_start  dev i32 [g + 1], ascending within 0 .. k;  src  dev i32 [k]
 * A target whose slot is outside 0 .. S-1 or whose group_old_row is >= ring is skipped, and so is a src entry outside 0 .. m-1; the entries of
 * group_start are clamped to 0 .. k.  Refused: a NaN alpha.  g = 0: returns 0 and launches nothing. */
int busca_store_ema_fit(float* gallery, int32_t S, int32_t ring, int32_t E, const float* feats, int32_t m, const int32_t* group_slot,
                        const int32_t* group_old_row, const int32_t* group_start, const int32_t* src, int32_t g, int32_t k, double alpha,
                        int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
