// The per-call context of the GEMM family (host only: no HIP header, no kernel; tools/callctx_host_check runs it against heap buffers).
// An entry point that takes a `precision` builds ONE CallCtx from its arguments and hands it down by reference: the launchers and shape
// queries of gemm.hip take it as a parameter without a default, so a helper called without a context does not compile.  It holds
//   - the product mode as the dispatch sees it: 0 f32 MFMA, 1 bf16-rounded operands, 2 fp32-accurate six-product bf16 split; ABI mode 3
//     (MLSP_PREC_F16X3) is seen as 2 with split_half(): two f16 pieces / three products on the launches gemm_split_kernel<.., NPC = 2> covers;
//   - the f16x3 operand bounds of this call: AMAX_PARTS partial maxima of |X| per operand, in a ring of slots in the last
//     MLSP_AMAX_TAIL_BYTES of the call's workspace (Workspace, common.h, never hands that tail out), with the operands measured or produced
//     so far (an operand is measured once per call: dgrad and weight gradient share dY);
//   - the caller's bounds table (include/mlsp_hip.h mlsp_operand_bounds_next): an operand that matches an entry uses the entry's partials --
//     as they are when `valid`, else this call measures INTO them and sets `valid` (the caller keeps them for later calls: the same
//     activation read by several layers, a weight read again by its layer's backward).
// Nothing outlives the call, and nothing is restored when it ends.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mlsp_hip.h"

#define MLSP_AMAX_TAIL_BYTES 65536
#define AMAX_PARTS 256
#define AMAX_SLOTS ((MLSP_AMAX_TAIL_BYTES - 256) / (AMAX_PARTS * 4))
struct AmaxOp { const float* X; long rows; int cols, ld; float* out; };
struct AmaxArgs { AmaxOp op[5]; };                    // what ONE measuring launch takes (gemm.hip amax_partials_kernel)
// queue of operands to measure with the next launch (launch_gemm batches A and B -- and the groups' B operands -- into one launch)
struct AmaxBatch { AmaxArgs args; int n = 0; };

// The ONE thread-local of the kernel library: the table that mlsp_operand_bounds_next arms for the next entry point this thread calls
// that takes a `precision`.  It exists because the ABI delivers that argument out of band (a real argument slot is an ABI bump); every
// CallCtx empties it as its first act, so it never outlives the call it was meant for.
struct PendingBounds { mlsp_bound_t* tab = nullptr; int n = 0; };
inline thread_local PendingBounds tl_pending_bounds;
static inline PendingBounds take_pending_bounds() { const PendingBounds t = tl_pending_bounds; tl_pending_bounds = PendingBounds(); return t; }

class CallCtx {
public:
    // a compute entry point: adopts the armed table; ws / ws_bytes: the call's workspace (a tail needs ws_bytes >= 2 * MLSP_AMAX_TAIL_BYTES;
    // without one mode 3 runs the bf16 pieces).  A bad `precision` still empties the slot: check ok() and return MLSP_ERR_ARG.
    CallCtx(int precision, void* ws, size_t ws_bytes) : CallCtx(precision, ws, ws_bytes, take_pending_bounds()) {}
    // an exported shape query: empties the slot and DROPS the table (the query is "the next entry point that takes a precision"); no tail
    static CallCtx query(int precision) { take_pending_bounds(); return CallCtx(precision, nullptr, 0, PendingBounds()); }
    CallCtx(const CallCtx&) = delete;
    CallCtx& operator=(const CallCtx&) = delete;

    bool ok() const { return ok_; }
    int mode() const { return mode_; }
    bool split_half() const { return split_half_; }
    bool has_tail() const { return base_ != nullptr; }

    // -> the partials of X [rows][cols] (pitch ld), measured now (queued into `batch`) or earlier in this call; null: cannot (no tail,
    // unaligned, the batch is full).  *n_out: how many partials they are
    float* get(AmaxBatch& batch, const float* X, long rows, int cols, int ld, int* n_out) {
        *n_out = AMAX_PARTS;
        if (!base_ || !aligned(X, rows, cols, ld)) return nullptr;
        for (int i = 0; i < noffered_; ++i) {
            mlsp_bound_t& o = offered_[i];
            if (!same(o, X, rows, cols, ld) || !o.partials || o.n < 0 || o.n > 4096) continue;
            if (!o.valid) {
                if (o.n != 0 && o.n != AMAX_PARTS) continue;            // (an unfilled OUTPUT-bounds buffer of another size: not ours to measure into)
                if (batch.n >= 5) return nullptr;
                batch.args.op[batch.n++] = {X, rows, cols, ld, o.partials};
                o.valid = 1; o.n = AMAX_PARTS;
            }
            *n_out = o.n ? o.n : AMAX_PARTS;
            return o.partials;
        }
        if (const AmaxOp* c = cached(X, rows, cols, ld)) return c->out;
        if (batch.n >= 5) return nullptr;
        float* out = take_slot(X, rows, cols, ld);
        batch.args.op[batch.n++] = {X, rows, cols, ld, out};
        return out;
    }
    // Is a bound of X at hand (a valid entry of the caller's table, or measured / produced earlier in this call)?  No side effects.
    bool at_hand(const float* X, long rows, int cols, int ld) const {
        for (int i = 0; i < noffered_; ++i) {
            const mlsp_bound_t& o = offered_[i];
            if (same(o, X, rows, cols, ld) && o.partials && o.valid && o.n > 0 && o.n <= 4096) return true;
        }
        return cached(X, rows, cols, ld) != nullptr;
    }
    // A slot for the partial maxima of X, FILLED BY THE CALLER's own kernels (the passes that write X, e.g. edge.hip edge_amax_raise) before
    // the product that reads X is launched in this same call: that product finds the slot like a measured one (an entry of the caller's
    // table for X is filled instead and marked valid: the caller hands it to later calls).  null: not an f16x3 call with a tail / X is not
    // an operand the products would look up / the caller's entry is valid already.
    float* reserve(const float* X, long rows, int cols, int ld) {
        if (!base_ || !split_half_ || !aligned(X, rows, cols, ld)) return nullptr;
        for (int i = 0; i < noffered_; ++i) {                 // the caller's own entry for X: filled there (and handed on by the caller), or already valid
            mlsp_bound_t& o = offered_[i];
            if (!same(o, X, rows, cols, ld)) continue;
            if (!o.partials || o.valid || (o.n != 0 && o.n != AMAX_PARTS)) return nullptr;
            o.valid = 1; o.n = AMAX_PARTS;
            return o.partials;
        }
        return take_slot(X, rows, cols, ld);
    }
    // An entry of the caller's table that describes an OUTPUT of this call (same pointer / shape, valid == 0, room for `need` floats): the
    // call fills its partials with a bound of what it writes -- e.g. the per-channel analytic bound of a BatchNorm'd layer -- and the
    // caller hands them to the layers that read the tensor.  -> the partials (entry marked valid, n = need), or null.
    float* offered_output(const float* out, long rows, int cols, int ld, int need) {
        for (int i = 0; i < noffered_; ++i) {
            mlsp_bound_t& o = offered_[i];
            if (!same(o, out, rows, cols, ld) || !o.partials || o.valid || o.n < need) continue;
            o.valid = 1; o.n = need;
            return o.partials;
        }
        return nullptr;
    }

private:
    CallCtx(int precision, void* ws, size_t ws_bytes, PendingBounds t)
        : ok_(precision >= 0 && precision <= 3), mode_(!ok_ ? 0 : precision == 3 ? 2 : precision), split_half_(precision == 3),
          base_((precision == 3 && ws && ws_bytes >= 2 * MLSP_AMAX_TAIL_BYTES)
                    ? (float*)((char*)ws + (ws_bytes - MLSP_AMAX_TAIL_BYTES + 255) / 256 * 256) : nullptr),
          offered_(t.tab), noffered_(t.n) {}
    static bool aligned(const float* X, long rows, int cols, int ld) {
        return rows > 0 && cols > 0 && !(cols & 3) && !(ld & 3) && !(((uintptr_t)X) & 15);
    }
    static bool same(const mlsp_bound_t& o, const float* X, long rows, int cols, int ld) {
        return o.ptr == X && o.rows == rows && o.cols == cols && o.ld == ld;
    }
    const AmaxOp* cached(const float* X, long rows, int cols, int ld) const {
        for (int i = 0; i < ncache_; ++i) {
            const AmaxOp& c = cache_[i];
            if (c.X == X && c.rows == rows && c.cols == cols && c.ld == ld) return &c;
        }
        return nullptr;
    }
    // the next slot of the ring, now X's; the slot's previous tenant leaves the cache
    float* take_slot(const float* X, long rows, int cols, int ld) {
        float* out = base_ + (size_t)next_ * AMAX_PARTS;
        next_ = (next_ + 1) % AMAX_SLOTS;
        int k = 0;
        for (int i = 0; i < ncache_; ++i) if (cache_[i].out != out) cache_[k++] = cache_[i];
        ncache_ = k;
        cache_[ncache_++] = {X, rows, cols, ld, out};
        return out;
    }

    const bool ok_;
    const int mode_;
    const bool split_half_;
    float* const base_;                 // the workspace tail (null: none)
    mlsp_bound_t* const offered_; const int noffered_;
    int next_ = 0, ncache_ = 0;
    AmaxOp cache_[AMAX_SLOTS];
};
