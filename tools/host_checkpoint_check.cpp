// Stand-alone check of apzh_game_save / apzh_game_load for a sanitizer build of the host library (CPU only; it is
// never loaded into Python and never needs a GPU):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       tools/host_checkpoint_check.cpp alphapig_amd/csrc/host_tree.cpp -o tools/_build/host_checkpoint_check
//   tools/_build/host_checkpoint_check
//
// It plays pools of 8 games (8x8 and 15x15) to a mid-search point with a closed-form evaluator, moves every game into a
// fresh pool through a blob, plays both pools to the end of the games side by side, and offers the damaged blobs of
// tests/test_pool_checkpoint.py (truncated, bumped magic, wrong board, first_child past the arena, action off the board,
// and bytes of the header and of the index arrays flipped one at a time) to a pool whose slot must stay as it was.
// Exit status 0 and "ok" on the last line: every comparison held and the sanitizers stayed silent.
#include "alphapig_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, apzh_last_error()); std::exit(1); } } while (0)

namespace {

typedef std::vector<uint8_t> Blob;

apzh_pool *make_pool(int side, int n_in_row, int n_playout, int n_games) {
    apzh_config c;
    std::memset(&c, 0, sizeof c);
    c.width = c.height = side; c.n_in_row = n_in_row; c.n_games = n_games; c.n_playout = n_playout;
    c.prior_is_f32 = 1; c.n_threads = 1; c.c_puct = 5.0;
    apzh_pool *p = apzh_create(&c);
    REQUIRE(p);
    for (int g = 0; g < n_games; g++) REQUIRE(apzh_game_reset(p, g, 0) == APZH_OK);
    return p;
}

// a peaked policy and a value in (-1, 1) from integer hashes of the code row
void evaluate(const uint8_t *codes, int hw, float *probs, float *value) {
    uint32_t h = 2166136261u;
    for (int m = 0; m <= hw; m++) h = (h ^ codes[m]) * 16777619u;
    double tot = 0.0;
    std::vector<double> w((size_t)hw);
    for (int m = 0; m < hw; m++) {
        uint32_t x = (h + (uint32_t)m * 2654435761u) % 1009u;
        w[m] = (double)(x + 1) * (double)(x + 1) * (x % 13 == 0 ? 40.0 : 1.0);
        tot += w[m];
    }
    for (int m = 0; m < hw; m++) probs[m] = (float)(w[m] / tot);
    *value = (float)((double)(h % 1601u) - 800.0) / 1000.0f;
}

Blob save(apzh_pool *p, int g) {
    int64_t n = apzh_game_save_size(p, g);
    REQUIRE(n > 0);
    Blob b((size_t)n);
    REQUIRE(apzh_game_save(p, g, b.data(), n - 1) < 0);         // a buffer one byte short is refused
    REQUIRE(apzh_game_save(p, g, b.data(), n) == n);
    return b;
}

// one round of game g on every pool: -> false once the game has ended.  The pools must agree in all they emit.
bool round(std::vector<apzh_pool *> &pools, int g, int side) {
    const int hw = side * side, stride = apzh_code_stride(side, side);
    std::vector<uint8_t> codes((size_t)stride), codes0;
    int32_t st0 = 0;
    for (size_t k = 0; k < pools.size(); k++) {
        int32_t st;
        REQUIRE(apzh_advance(pools[k], &g, 1, &st, codes.data()) == APZH_OK);
        if (k == 0) { st0 = st; codes0 = codes; }
        REQUIRE(st == st0 && (st != APZH_NEED_EVAL || codes == codes0));
    }
    if (st0 == APZH_NEED_EVAL) {
        std::vector<float> probs((size_t)hw);
        float value;
        evaluate(codes0.data(), hw, probs.data(), &value);
        for (apzh_pool *p : pools) REQUIRE(apzh_feed(p, &g, 1, probs.data(), &value) == APZH_OK);
        return true;
    }
    std::vector<int32_t> v0((size_t)hw), v((size_t)hw);
    int32_t out0[3] = {0, 0, 0};
    int move = 0;
    for (size_t k = 0; k < pools.size(); k++) {
        REQUIRE(apzh_root_visits_dense(pools[k], &g, 1, v.data(), nullptr) == APZH_OK);
        if (k == 0) {
            v0 = v;
            for (int m = 1; m < hw; m++) if (v0[m] > v0[move]) move = m;
        }
        REQUIRE(v == v0);
        int32_t out[3];
        REQUIRE(apzh_play_move(pools[k], g, move, out) == APZH_OK);
        if (k == 0) std::memcpy(out0, out, sizeof out);
        REQUIRE(std::memcmp(out, out0, sizeof out) == 0);
    }
    return out0[0] == 0;
}

void check_board(int side, int n_in_row, int n_playout, int other_side, int other_row) {
    const int hw = side * side;
    apzh_pool *a = make_pool(side, n_in_row, n_playout, 8);
    std::vector<apzh_pool *> one{a};
    std::vector<uint8_t> pending_codes[6];
    // games 0 .. 5 into the search of their third move and on to a pending leaf, 6 right behind its first move, 7 empty
    for (int g = 0; g < 6; g++) {
        for (int r = 0; r < 2 * (n_playout + 1) + n_playout / 2; r++) REQUIRE(round(one, g, side));
        int32_t st;
        pending_codes[g].resize((size_t)apzh_code_stride(side, side));
        REQUIRE(apzh_advance(a, &g, 1, &st, pending_codes[g].data()) == APZH_OK && st == APZH_NEED_EVAL);
    }
    for (int r = 0; r < n_playout + 1; r++) REQUIRE(round(one, 6, side));
    REQUIRE(apzh_playouts_done(a, 6) == 0);
    apzh_pool *b = make_pool(side, n_in_row, n_playout, 8);
    std::vector<Blob> blobs;
    for (int g = 0; g < 8; g++) {
        blobs.push_back(save(a, g));
        REQUIRE(apzh_game_load(b, g, blobs[g].data(), (int64_t)blobs[g].size()) == APZH_OK);
        REQUIRE(save(b, g) == blobs[g]);
    }
    // damaged blobs against slots 2 (pending leaf), 6 (between moves) and 7 (empty): refused, the slot untouched
    const Blob &good = blobs[2];
    int32_t counts[3];
    std::memcpy(counts, good.data() + 52, sizeof counts);
    const size_t arena = 88 + 3 * (size_t)hw + 3 * (size_t)counts[0] + 2 * (size_t)counts[1], n = (size_t)counts[2];
    REQUIRE(n > 4 && good.size() == arena + 33 * n);
    std::vector<Blob> bad;
    bad.push_back(Blob(good.begin(), good.end() - 1));
    bad.push_back(Blob(good.begin(), good.begin() + (long)good.size() / 2));
    bad.push_back(Blob());
    { Blob x = good; x[0] += 1; bad.push_back(x); }
    { Blob x = good; x[8] += 1; bad.push_back(x); }
    { Blob x = good; int32_t v = (int32_t)n; std::memcpy(x.data() + arena + 4 * n, &v, 4); bad.push_back(x); }
    { Blob x = good; int16_t v = (int16_t)hw; std::memcpy(x.data() + arena + 14 * n + 2 * 3, &v, 2); bad.push_back(x); }
    {
        apzh_pool *o = make_pool(other_side, other_row, n_playout, 1);
        bad.push_back(save(o, 0));
        REQUIRE(apzh_game_load(o, 0, good.data(), (int64_t)good.size()) < 0);
        apzh_destroy(o);
    }
    const int slots[3] = {2, 6, 7};
    for (const Blob &x : bad)
        for (int g : slots) {
            const Blob before = save(b, g);
            REQUIRE(apzh_game_load(b, g, x.empty() ? nullptr : x.data(), (int64_t)x.size()) < 0);
            REQUIRE(apzh_last_error()[0] != 0 && save(b, g) == before);
        }
    // bytes of the header's checked fields and of the parent / first_child / n_child / action arrays, all bits of one
    // byte flipped at a time: the load either refuses the blob or accepts one that is consistent -- into a scratch pool, which then plays
    // a few rounds on it; no outcome may touch memory it does not own
    apzh_pool *s = make_pool(side, n_in_row, n_playout, 1);
    std::vector<size_t> spots;
    for (size_t i = 0; i < 64; i++) spots.push_back(i);
    const size_t step = (12 * n / 4000) | 1;                    // (odd: every byte lane of the indices gets its turn)
    for (size_t i = arena; i < arena + 16 * n; i += step)
        if (i < arena + 8 * n || i >= arena + 12 * n) spots.push_back(i);
    size_t refused = 0;
    for (size_t i : spots) {
        Blob x = good;
        x[i] ^= 0xff;
        if (apzh_game_load(s, 0, x.data(), (int64_t)x.size()) < 0) { refused++; continue; }
        const float value = 0.25f;
        const std::vector<float> probs((size_t)hw, 1.0f / (float)hw);
        const int g0 = 0;
        for (int r = 0; r < 6; r++) {
            int32_t st;
            REQUIRE(apzh_advance(s, &g0, 1, &st, nullptr) == APZH_OK);
            if (st != APZH_NEED_EVAL) break;
            REQUIRE(apzh_feed(s, &g0, 1, probs.data(), &value) == APZH_OK);
        }
    }
    std::printf("%dx%d: %zu of %zu flipped bytes refused\n", side, side, refused, spots.size());
    REQUIRE(refused > 0 && refused < spots.size());
    apzh_destroy(s);
    // both pools to the end of every game
    std::vector<apzh_pool *> both{a, b};
    for (int g = 0; g < 8; g++) {
        if (g < 6) {
            std::vector<float> probs((size_t)hw);
            float value;
            evaluate(pending_codes[g].data(), hw, probs.data(), &value);
            for (apzh_pool *p : both) REQUIRE(apzh_feed(p, &g, 1, probs.data(), &value) == APZH_OK);
        }
        int rounds = 0;
        while (round(both, g, side)) REQUIRE(++rounds < 1000000);
        int32_t sa[5], sb[5];
        REQUIRE(apzh_game_status(a, g, sa) == APZH_OK && apzh_game_status(b, g, sb) == APZH_OK);
        REQUIRE(std::memcmp(sa, sb, sizeof sa) == 0 && sa[2] == 1);
        REQUIRE(save(a, g) == save(b, g));
    }
    apzh_destroy(a);
    apzh_destroy(b);
}

}  // namespace

int main() {
    check_board(8, 4, 16, 15, 5);
    check_board(15, 5, 24, 8, 4);
    std::printf("ok\n");
    return 0;
}
