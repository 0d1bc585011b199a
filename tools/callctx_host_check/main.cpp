// Host check of the per-call context of the GEMM family (mlsp_amd/csrc/callctx.h): the f16x3 operand-bound bookkeeping -- the slot ring in
// the workspace tail, the measured-operand cache, the caller's table, the one pending slot -- run against heap buffers of exactly the
// sizes the library uses: a workspace of exactly 2 * MLSP_AMAX_TAIL_BYTES (the smallest with a tail), entries of exactly 256 floats.  Every
// slot the context hands out is written end to end, so an address past either end of anything is an AddressSanitizer report.
// A stand-alone program that needs no GPU and no HIP header:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/callctx_host_check/main.cpp
//       -o build/callctx_host_check && build/callctx_host_check
#include "../../mlsp_amd/csrc/callctx.h"
#include <stdio.h>
#include <stdlib.h>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// exact-size, 256-byte-aligned heap array
template <typename T>
struct Buf {
    T* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void**)&p, 256, (n ? n : 1) * sizeof(T))) abort(); for (size_t i = 0; i < n; ++i) p[i] = T(0); }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};
static void fill_slot(float* s, float v) { for (int i = 0; i < AMAX_PARTS; ++i) s[i] = v; }
static void arm(mlsp_bound_t* tab, int n) { tl_pending_bounds.tab = tab; tl_pending_bounds.n = n; }      // what mlsp_operand_bounds_next does

int main() {
    const size_t WS = 2 * MLSP_AMAX_TAIL_BYTES;
    Buf<char> ws(WS);
    Buf<float> X(4 * 80);                          // operand i: the aligned quad at X.p + 4 i, shape [1][4]
    float* const tail = (float*)(ws.p + WS - MLSP_AMAX_TAIL_BYTES);
    int n = -1;

    {   // the modes as the dispatch sees them; a bad precision
        CallCtx a(0, ws.p, WS), b(1, ws.p, WS), c(2, ws.p, WS), d(3, ws.p, WS), e(7, ws.p, WS), f(-1, nullptr, 0);
        EXPECT(a.ok() && a.mode() == 0 && !a.split_half() && !a.has_tail());
        EXPECT(b.ok() && b.mode() == 1 && !b.split_half() && !b.has_tail());
        EXPECT(c.ok() && c.mode() == 2 && !c.split_half() && !c.has_tail());
        EXPECT(d.ok() && d.mode() == 2 && d.split_half() && d.has_tail());
        EXPECT(!e.ok() && !f.ok());
    }
    {   // a context with no tail answers null everywhere: no workspace, one byte too few, a query
        CallCtx a(3, nullptr, 0), b(3, ws.p, WS - 1);
        const CallCtx q = CallCtx::query(3);
        CallCtx* all[2] = {&a, &b};
        for (CallCtx* cx : all) {
            AmaxBatch batch;
            EXPECT(cx->ok() && cx->mode() == 2 && cx->split_half() && !cx->has_tail());
            EXPECT(!cx->get(batch, X.p, 1, 4, 4, &n) && batch.n == 0 && !cx->reserve(X.p, 1, 4, 4) && !cx->at_hand(X.p, 1, 4, 4));
            EXPECT(!cx->offered_output(X.p, 1, 4, 4, 4));
        }
        EXPECT(q.ok() && q.mode() == 2 && !q.has_tail() && !q.at_hand(X.p, 1, 4, 4));
    }
    {   // the ring: AMAX_SLOTS distinct slots inside the tail, then it wraps and the evicted tenant leaves the cache
        CallCtx cx(3, ws.p, WS);
        EXPECT(AMAX_SLOTS == 63);
        for (int i = 0; i < AMAX_SLOTS; ++i) {
            float* s = cx.reserve(X.p + 4 * i, 1, 4, 4);
            EXPECT(s == tail + (size_t)i * AMAX_PARTS);
            if (s) fill_slot(s, (float)i);
        }
        AmaxBatch batch;
        EXPECT(cx.at_hand(X.p, 1, 4, 4) && cx.get(batch, X.p, 1, 4, 4, &n) == tail && n == AMAX_PARTS && batch.n == 0);     // found, not measured again
        EXPECT(!cx.at_hand(X.p, 1, 8, 8) && !cx.at_hand(X.p, 2, 4, 4));                     // (keyed by pointer AND shape)
        float* s = cx.reserve(X.p + 4 * AMAX_SLOTS, 1, 4, 4);
        EXPECT(s == tail);
        if (s) fill_slot(s, -1.f);
        EXPECT(!cx.at_hand(X.p, 1, 4, 4) && cx.at_hand(X.p + 4, 1, 4, 4) && cx.at_hand(X.p + 4 * AMAX_SLOTS, 1, 4, 4));
        EXPECT(cx.get(batch, X.p, 1, 4, 4, &n) == tail + AMAX_PARTS && batch.n == 1 && batch.args.op[0].X == X.p && batch.args.op[0].out == tail + AMAX_PARTS);
        EXPECT(!cx.at_hand(X.p + 4, 1, 4, 4) && cx.at_hand(X.p, 1, 4, 4));                 // (operand 1 was that slot's tenant)
        // what the products would not look up: unaligned, ragged, empty
        EXPECT(!cx.reserve(X.p + 1, 1, 4, 4) && !cx.reserve(X.p, 1, 6, 8) && !cx.reserve(X.p, 1, 4, 6) && !cx.reserve(X.p, 0, 4, 4) && !cx.reserve(X.p, 1, 0, 4));
        EXPECT(!cx.get(batch, X.p + 1, 1, 4, 4, &n) && !cx.get(batch, X.p, 1, 6, 8, &n) && !cx.get(batch, X.p, 1, 4, 6, &n) && !cx.get(batch, X.p, 0, 4, 4, &n) && batch.n == 1);
    }
    {   // a bf16x6 call reserves nothing, even with a workspace
        CallCtx cx(2, ws.p, WS);
        EXPECT(!cx.reserve(X.p, 1, 4, 4));
    }
    {   // a sixth operand in one batch is refused (and takes no slot)
        CallCtx cx(3, ws.p, WS);
        AmaxBatch batch;
        for (int i = 0; i < 5; ++i) EXPECT(cx.get(batch, X.p + 4 * i, 1, 4, 4, &n) == tail + (size_t)i * AMAX_PARTS && batch.n == i + 1);
        EXPECT(!cx.get(batch, X.p + 20, 1, 4, 4, &n) && batch.n == 5 && !cx.at_hand(X.p + 20, 1, 4, 4));
        EXPECT(cx.get(batch, X.p + 8, 1, 4, 4, &n) == tail + 2 * AMAX_PARTS && batch.n == 5);           // (one already queued is still found)
        batch.n = 0;                                                                       // (flushed)
        EXPECT(cx.get(batch, X.p + 20, 1, 4, 4, &n) == tail + 5 * AMAX_PARTS && batch.n == 1);
    }
    {   // the caller's table
        Buf<float> pa(AMAX_PARTS), pb(17), pc(128), pd(64), pe(AMAX_PARTS);
        mlsp_bound_t tab[5] = {
            {X.p, 1, 4, 4, pa.p, 0, 0},             // to be measured
            {X.p + 4, 1, 4, 4, pb.p, 1, 17},        // valid, 17 partials of the caller's own
            {X.p + 8, 1, 4, 4, pc.p, 0, 128},       // an unfilled output buffer of another size
            {X.p + 12, 1, 4, 4, pd.p, 0, 64},       // room for an output bound of 64 floats
            {X.p + 16, 1, 4, 4, pe.p, 0, 256},      // to be filled by the caller's own kernels
        };
        arm(tab, 5);
        CallCtx cx(3, ws.p, WS);
        EXPECT(!tl_pending_bounds.tab && tl_pending_bounds.n == 0);                        // adopted: the slot is empty
        AmaxBatch batch;
        // valid = 0: queued into the batch, measured INTO the entry, marked
        EXPECT(!cx.at_hand(X.p, 1, 4, 4));
        EXPECT(cx.get(batch, X.p, 1, 4, 4, &n) == pa.p && n == AMAX_PARTS && batch.n == 1 && batch.args.op[0].out == pa.p && batch.args.op[0].X == X.p);
        EXPECT(tab[0].valid == 1 && tab[0].n == AMAX_PARTS && cx.at_hand(X.p, 1, 4, 4));
        fill_slot(pa.p, 1.f);
        EXPECT(cx.get(batch, X.p, 1, 4, 4, &n) == pa.p && n == AMAX_PARTS && batch.n == 1);           // now valid: used as it is
        EXPECT(!cx.reserve(X.p, 1, 4, 4));                                                 // (valid already: nothing to fill)
        // valid = 1: returned untouched, with its own n
        EXPECT(cx.at_hand(X.p + 4, 1, 4, 4));
        EXPECT(cx.get(batch, X.p + 4, 1, 4, 4, &n) == pb.p && n == 17 && batch.n == 1 && tab[1].valid == 1 && tab[1].n == 17);
        // valid = 0 with n other than 0 or 256: get measures into a slot of its own, reserve refuses
        EXPECT(!cx.reserve(X.p + 8, 1, 4, 4) && tab[2].valid == 0 && tab[2].n == 128);
        EXPECT(cx.get(batch, X.p + 8, 1, 4, 4, &n) == tail && n == AMAX_PARTS && batch.n == 2 && tab[2].valid == 0 && tab[2].n == 128);
        // offered_output demands n >= need
        EXPECT(!cx.offered_output(X.p + 12, 1, 4, 4, 128) && tab[3].valid == 0 && tab[3].n == 64);
        EXPECT(!cx.offered_output(X.p + 12, 2, 4, 4, 64));
        EXPECT(cx.offered_output(X.p + 12, 1, 4, 4, 32) == pd.p && tab[3].valid == 1 && tab[3].n == 32);
        EXPECT(!cx.offered_output(X.p + 12, 1, 4, 4, 32));                                 // (valid now)
        EXPECT(cx.get(batch, X.p + 12, 1, 4, 4, &n) == pd.p && n == 32 && batch.n == 2);
        // reserve fills the caller's own entry for X
        EXPECT(cx.reserve(X.p + 16, 1, 4, 4) == pe.p && tab[4].valid == 1 && tab[4].n == AMAX_PARTS);
        fill_slot(pe.p, 2.f);
        // the table was for that call only
        CallCtx next(3, ws.p, WS);
        AmaxBatch b2;
        EXPECT(!next.at_hand(X.p + 4, 1, 4, 4) && next.get(b2, X.p + 4, 1, 4, 4, &n) == tail && b2.n == 1);
    }
    {   // query() drops an armed table; so does a call with a bad precision
        Buf<float> pa(AMAX_PARTS);
        mlsp_bound_t tab[1] = {{X.p, 1, 4, 4, pa.p, 0, 0}};
        for (int bad = 0; bad < 2; ++bad) {
            arm(tab, 1);
            if (bad) { CallCtx e(7, ws.p, WS); EXPECT(!e.ok()); }
            else EXPECT(CallCtx::query(3).ok());
            EXPECT(!tl_pending_bounds.tab && tl_pending_bounds.n == 0);
            CallCtx cx(3, ws.p, WS);
            AmaxBatch batch;
            EXPECT(cx.get(batch, X.p, 1, 4, 4, &n) == tail && tab[0].valid == 0 && tab[0].n == 0);
        }
    }
    printf("callctx_host_check: %s (modes, no tail, ring of %d slots, batch limit, caller's table, pending slot)\n", fails ? "FAILED" : "ok", AMAX_SLOTS);
    return fails != 0;
}
