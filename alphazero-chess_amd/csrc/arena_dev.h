// arena_dev.h -- the rules of a ply of an evaluation game (validation.rs:284-402), apart from the match
// engine's bookkeeping in arena.hip, whose pick and commit kernels call them:
//   arena_pick    legal moves of the position and the mover's choice among them -- a policy row under
//                 validation.rs:297-308, a uniform entry of the legal-move list, or a given action -- and
//                 its validation
//   arena_commit  play_move (chess.rs:36-63) of the chosen index and the appends to the histories
// Both run on one wavefront per game (blockDim 64); every lane returns the same values.
#pragma once
#include "az_internal.h"
#include "search_dev.h"

namespace azi {

enum { ST_OK = 0, ST_ILLEGAL = 1, ST_NONFINITE = 2 };

struct PickShared {
    Edge ed[MAX_EDGES];
    float w[MAX_EDGES];
    float sw[MAX_EDGES];
    uint16_t si[MAX_EDGES];
    int a;
};

__device__ __forceinline__ bool non_finite(float w) { return (azc::f2u(w) & 0x7f800000u) == 0x7f800000u; }

// The choice of the mover of position p.  pol: the mover's policy row [4096] (a base-model player's network
// output, or an MCTS player's improved policy: 0 off the legal indices), or nullptr; without a row, kind
// AZ_PLAYER_RANDOM draws entry min(floor(u n), n - 1) of the legal-move list and every other kind plays
// `given`.  Returns the move index; *st = ST_OK, or why the step must be refused.
__device__ __forceinline__ int arena_pick(PickShared& S, azc::Pos p, int kind, const float* __restrict__ pol, float u,
                                          int given, int nsm, int lane, int* st_out) {
    int n = 0;
    leaf_rules<1>(p, S.ed, lane, &n);
    __syncthreads();
    int action = -1, st = ST_OK;
    if (pol) {
        bool bad = false;
        float bw = -1.0f;
        int bi = -1;
        for (int e = lane; e < n; e += 64) {
            const int ii = S.ed[e].idx & azc::IDX_MASK;
            const float w = pol[ii];
            S.w[e] = w;
            bad |= non_finite(w);
            if (w > bw || (w == bw && ii > bi)) { bw = w; bi = ii; }
        }
        if (__ballot(bad)) {
            st = ST_NONFINITE;
        } else if ((int)p.fullmoves > nsm) {                 // validation.rs:297: the LAST maximal index
            for (int o = 32; o > 0; o >>= 1) {
                const float ow = __shfl_xor(bw, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ow > bw || (ow == bw && oi > bi)) { bw = ow; bi = oi; }
            }
            action = bw > 0.0f ? bi : AZ_ACTION_SPACE - 1;   // an all-zero row's last maximum is entry 4095
        } else {                                             // WeightedIndex: ascending index order
            __syncthreads();
            for (int e = lane; e < n; e += 64) {
                const int ii = S.ed[e].idx & azc::IDX_MASK;
                int r = 0;
                for (int f = 0; f < n; f++) r += (S.ed[f].idx & azc::IDX_MASK) < ii;
                S.si[r] = (uint16_t)ii;
                S.sw[r] = S.w[e];
            }
            __syncthreads();
            if (lane == 0) {
                float total = 0.0f;
                for (int r = 0; r < n; r++) total = total + S.sw[r];
                float x = u * total;
                if (!(x < total)) x = nextafterf(total, 0.0f);
                float cw = 0.0f;
                int a = AZ_ACTION_SPACE - 1;                 // no cumulative weight above x: the last entry
                for (int r = 0; r < n; r++) {
                    cw = cw + S.sw[r];
                    if (cw > x) { a = S.si[r]; break; }
                }
                S.a = a;
            }
            __syncthreads();
            action = S.a;
        }
    } else if (kind == AZ_PLAYER_RANDOM) {                   // entry min(floor(u n), n - 1) of the list
        if (lane == 0) {                                     // with its under-promotion duplicates
            int tot = 0;
            for (int e = 0; e < n; e++) tot += (S.ed[e].idx & azc::PROMO_FLAG) ? 4 : 1;
            int k = (int)floorf(u * (float)tot);
            k = k < tot - 1 ? k : tot - 1;
            int a = -1, acc = 0;
            for (int e = 0; e < n; e++) {
                acc += (S.ed[e].idx & azc::PROMO_FLAG) ? 4 : 1;
                if (k < acc) { a = S.ed[e].idx & azc::IDX_MASK; break; }
            }
            S.a = a;
        }
        __syncthreads();
        action = S.a;
    } else {
        action = given;
    }
    if (st == ST_OK) {
        bool hit = false;
        for (int e = lane; e < n; e += 64) hit |= (S.ed[e].idx & azc::IDX_MASK) == action;
        if (!__ballot(hit)) st = ST_ILLEGAL;
    }
    *st_out = st;
    return action;
}

// play_move of `action` on hist[k], the position after k moves of a game whose position history is hist
// [HMAX] and whose move list is moves [HMAX]: outcome() first (chess.rs:43-50), then the repetition count
// against the history, then the 50-move, 200-fullmove and HMAX limits.  Lane 0 appends the new position
// and the move.  Returns the result; *turn = the side to move afterwards.
__device__ __forceinline__ int arena_commit(Edge* s_ed, azc::Pos* hist, int* moves, int k, int action, int lane,
                                            int* turn) {
    const azc::Pos p = hist[k];
    azc::Pos c = azc::play_index(p, action);
    int n = 0;
    int res = leaf_rules<1>(c, s_ed, lane, &n);
    if (res == azc::ONGOING) {
        // the position enters the multiset, then the draws (chess.rs:52-60): equal positions lie an
        // even number d <= halfmoves of plies back -- one candidate per lane
        const int hm = c.halfmoves;
        int cnt = 0;
        for (int d0 = 2; d0 <= hm; d0 += 128) {
            const int d = d0 + 2 * lane;
            bool eq = false;
            if (d <= hm && k + 1 - d >= 0) eq = azc::chess_eq(hist[k + 1 - d], c);
            cnt += __popcll(__ballot(eq));
        }
        if (cnt + 1 >= azc::REPETITIONS || c.halfmoves >= azc::NUM_HALFMOVES || c.fullmoves >= azc::NUM_FULLMOVES ||
            k + 1 >= HMAX)
            res = azc::DRAW;
    }
    if (lane == 0) {
        if (k + 1 < HMAX) hist[k + 1] = c;
        if (k < HMAX) moves[k] = action;
    }
    *turn = c.turn;
    return res;
}

}  // namespace azi
