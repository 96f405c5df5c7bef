// CPU-only exercise of the engine's HIP-free host logic (velocycle_amd/csrc/vc_host_logic.h) for AddressSanitizer / UBSan
// (tests/test_host_logic_sanitize_cpu.py builds this with g++ -fsanitize=address,undefined: sanitizers are not
// available on the GPU pool, so the host half is checked here).  Exits non-zero on any mismatch.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "../velocycle_amd/csrc/vc_host_logic.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the device pass, restated on the host: dense per-gene tables + overflow list, in an arbitrary (shuffled) order
static void device_like(const std::vector<float>& M, long long gs, long long cs, int Ng, int Nc, std::vector<unsigned>& tab,
                        std::vector<std::pair<int, float>>& ovf, bool& bad, std::mt19937& rng) {
  tab.assign((size_t)Ng * VC_HIST_CAP, 0u);
  std::vector<std::pair<int, int>> order;
  for (int g = 0; g < Ng; ++g) for (int c = 0; c < Nc; ++c) order.push_back({g, c});
  std::shuffle(order.begin(), order.end(), rng);
  for (auto gc : order) {
    const float v = M[(size_t)gc.first * gs + (size_t)gc.second * cs];
    if (!vc_count_ok(v)) { bad = true; continue; }
    if (v == 0.f) continue;
    if (vc_count_dense(v)) tab[(size_t)gc.first * VC_HIST_CAP + (int)v]++;
    else ovf.push_back({gc.first, v});
  }
}

static void one_case(int Ng, int Nc, bool gene_major, bool spiky, unsigned seed) {
  std::mt19937 rng(seed);
  std::poisson_distribution<int> pois(1.3);
  const long long gs = gene_major ? Nc : 1, cs = gene_major ? 1 : Ng;
  std::vector<float> S((size_t)Ng * Nc), U((size_t)Ng * Nc);
  for (auto* M : {&S, &U})
    for (auto& v : *M) {
      v = (float)pois(rng);
      if (spiky && rng() % 97 == 0) v = (float)(2000 + rng() % 100000);
      if (spiky && rng() % 101 == 0) v = 0.25f + (float)(rng() % 64) * 0.5f;
    }
  std::vector<int> ptr_h, ptr_d;
  std::vector<float> val_h, cnt_h, val_d, cnt_d;
  bool bad_h = false, bad_d = false;
  const double lgS = vc_build_hist_host(S.data(), gs, cs, Ng, Nc, ptr_h, val_h, cnt_h, &bad_h);
  const double lgU = vc_build_hist_host(U.data(), gs, cs, Ng, Nc, ptr_h, val_h, cnt_h, &bad_h);
  ptr_h.push_back((int)val_h.size());
  double lgd[2];
  int m = 0;
  for (auto* M : {&S, &U}) {
    std::vector<unsigned> tab;
    std::vector<std::pair<int, float>> ovf;
    device_like(*M, gs, cs, Ng, Nc, tab, ovf, bad_d, rng);
    lgd[m++] = vc_compact_hist(tab.data(), Ng, ovf, ptr_d, val_d, cnt_d);
  }
  ptr_d.push_back((int)val_d.size());
  CHECK(!bad_h && !bad_d);
  CHECK(ptr_h == ptr_d && val_h == val_d && cnt_h == cnt_d);
  CHECK(std::fabs(lgS - lgd[0]) <= 1e-9 * (1.0 + std::fabs(lgS)) && std::fabs(lgU - lgd[1]) <= 1e-9 * (1.0 + std::fabs(lgU)));
  CHECK((int)ptr_h.size() == 2 * Ng + 1);
  // multiplicities add up to the non-zero entries; values strictly increase inside the dense part of a gene
  double total = 0;
  for (float c : cnt_h) total += c;
  double nz = 0;
  for (auto* M : {&S, &U}) for (float v : *M) nz += v != 0.f;
  CHECK(total == nz);
  std::vector<int> task, tptr;
  vc_build_hist_tasks(ptr_h, Ng, task, tptr);
  CHECK((int)tptr.size() == Ng + 1 && tptr.back() == (int)task.size() / 4);
  long long covered = 0;
  for (size_t t = 0; t + 3 < task.size(); t += 4) {
    CHECK(task[t] >= 0 && task[t] < Ng && (task[t + 1] == 0 || task[t + 1] == 1));
    CHECK(task[t + 3] - task[t + 2] >= 1 && task[t + 3] - task[t + 2] <= 64);
    CHECK(task[t + 2] >= ptr_h[(size_t)task[t + 1] * Ng + task[t]] && task[t + 3] <= ptr_h[(size_t)task[t + 1] * Ng + task[t] + 1]);
    covered += task[t + 3] - task[t + 2];
  }
  CHECK(covered == (long long)val_h.size());
}

// The cell tiling of the likelihood kernel: for every gene block the waves' ranges [first, first + cw) clamped to Nc, taken in
// the order (chunk, wave), tile [0, Nc) exactly -- no gap, no overlap -- whatever the shares, the number of gene blocks
// (also when it does not divide the CUs), the occupancy; and the grid never exceeds the resident slots when shares apply.
static void tiling_case(long long Nc, int nGB, int n_cu, int bpc, const double* share, int min_cw, long long cw_override) {
  const int waves = 4;
  const VcTiling t = vc_tile_cells(Nc, nGB, n_cu, bpc, waves, cw_override, share, min_cw);
  CHECK(t.n_chunks >= 1 && t.cw >= 1);
  bool unequal = false;
  for (int p = 1; p < 4; ++p) unequal |= t.pass_cw[p] != t.pass_cw[0];
  if (unequal) CHECK((long long)nGB * t.n_chunks <= (long long)bpc * n_cu);
  for (int p = 0; p < 4; ++p) CHECK(t.pass_cw[p] >= 1 && t.pass_cw[p] <= t.cw);
  for (int gb = 0; gb < nGB; ++gb) {
    long long next = 0;                    // first cell nobody has taken yet
    for (int chunk = 0; chunk < t.n_chunks; ++chunk)
      for (int w = 0; w < waves; ++w) {
        int cw = 0;
        long long b = vc_wave_first_cell(chunk, gb, w, nGB, n_cu, t.pass_cw, waves, &cw);
        long long e = b + cw;
        CHECK(cw >= 1);
        if (b > Nc) b = Nc;
        if (e > Nc) e = Nc;
        if (b < Nc) CHECK(b == next);
        if (e > next) next = e;
      }
    CHECK(next == Nc);
  }
}

// one-hot batches: order by batch, batch-aligned workgroup table -- every position of every gene block is covered exactly once,
// every workgroup lies inside the batch the table names, the batches' chunk ranges are consecutive and complete
static void batch_case(long long Nc, int Nb, int nGB, int n_cu, int bpc, bool shuffled, unsigned seed) {
  std::mt19937 rng(seed);
  std::vector<float> Db((size_t)Nb * Nc, 0.f);
  std::vector<int> want((size_t)Nc);
  for (long long c = 0; c < Nc; ++c) {
    int q = shuffled ? (int)(rng() % Nb) : (int)((c * Nb) / Nc);
    if (Nb > 2 && q == 1) q = 0;                 // an empty batch
    want[(size_t)c] = q;
    Db[(size_t)q * Nc + c] = 1.f;
  }
  std::vector<int> bid, pos, ord, len;
  CHECK(vc_onehot_batches(Db.data(), Nb, Nc, bid));
  CHECK(bid == want);
  const bool sorted = vc_order_by_batch(bid, Nb, pos, ord, len);
  if (!shuffled) CHECK(sorted);
  long long tot = 0;
  for (int q = 0; q < Nb; ++q) tot += len[(size_t)q];
  CHECK(tot == Nc);
  for (long long c = 0; c < Nc; ++c) CHECK(ord[(size_t)pos[(size_t)c]] == (int)c);
  for (long long p = 1; p < Nc; ++p) {
    CHECK(bid[(size_t)ord[(size_t)p]] >= bid[(size_t)ord[(size_t)p - 1]]);
    if (bid[(size_t)ord[(size_t)p]] == bid[(size_t)ord[(size_t)p - 1]]) CHECK(ord[(size_t)p] > ord[(size_t)p - 1]);      // stable
  }
  const double half[4] = {1.0, 0.5, 0.25, 0.125};
  VcTiling t = vc_tile_cells(Nc, nGB, n_cu, bpc, 4, 0, half, 12);
  int nonempty = 0;
  for (int v : len) nonempty += v > 0;
  if (t.n_chunks < nonempty) t.n_chunks = nonempty;
  std::vector<int> tile, bc;
  const int cwm = vc_tile_batches(Nc, nGB, t.n_chunks, n_cu, t.pass_cw, 4, len, tile, bc);
  std::vector<long long> start((size_t)Nb + 1, 0);
  for (int q = 0; q < Nb; ++q) start[(size_t)q + 1] = start[(size_t)q] + len[(size_t)q];
  for (int gb = 0; gb < nGB; ++gb) {
    long long next = 0;
    for (int k = 0; k < t.n_chunks; ++k) {
      const int* w = &tile[4 * ((size_t)k * nGB + gb)];
      const int q = w[2];
      CHECK(q >= 0 && q < Nb && w[1] <= cwm && w[1] >= 0);
      CHECK(k >= bc[(size_t)gb * (Nb + 1) + q] && k < bc[(size_t)gb * (Nb + 1) + q + 1]);
      CHECK(w[0] >= start[(size_t)q] && w[3] <= start[(size_t)q + 1] && w[0] <= w[3]);
      CHECK(w[0] == next || w[0] == w[3]);
      CHECK((long long)w[1] * 4 >= w[3] - w[0]);            // four waves of cw cells reach the end
      if (w[3] > w[0]) next = w[3];
    }
    CHECK(next == Nc);
    CHECK(bc[(size_t)gb * (Nb + 1)] == 0 && bc[(size_t)gb * (Nb + 1) + Nb] == t.n_chunks);
    for (int q = 0; q < Nb; ++q) CHECK(bc[(size_t)gb * (Nb + 1) + q] <= bc[(size_t)gb * (Nb + 1) + q + 1]);
  }
  // not one-hot: a fractional entry, two entries in one column, an empty column
  if (Nc >= 2) {
    std::vector<float> bad = Db;
    bad[0] = bad[0] == 1.f ? 0.5f : bad[0];
    for (int q = 0; q < Nb; ++q) if (bad[(size_t)q * Nc] == 1.f) bad[(size_t)q * Nc] = 0.5f;
    CHECK(!vc_onehot_batches(bad.data(), Nb, Nc, bid));
    bad = Db;
    for (int q = 0; q < Nb; ++q) bad[(size_t)q * Nc + 1] = 0.f;
    CHECK(!vc_onehot_batches(bad.data(), Nb, Nc, bid));
    if (Nb >= 2) { bad = Db; bad[1] = 1.f; bad[(size_t)Nc + 1] = 1.f; CHECK(!vc_onehot_batches(bad.data(), Nb, Nc, bid)); }
  }
}

// the condition of every batch (vc_batch_conditions): D is (Nx, Nc) row-major, bid the batch of every cell
static void condition_cases() {
  std::vector<int> cond;
  // one condition per batch: batches 0 and 2 in condition 1, batch 1 in condition 0
  {
    const std::vector<int> bid = {0, 1, 2, 0, 1, 2};
    const std::vector<float> D = {0, 1, 0, 0, 1, 0,
                                  1, 0, 1, 1, 0, 1};
    CHECK(vc_batch_conditions(D.data(), 2, 6, bid, 3, cond));
    CHECK((cond == std::vector<int>{1, 0, 1}));
  }
  // a batch that mixes conditions: cells 0 and 2 are both batch 0, in conditions 0 and 1
  {
    const std::vector<int> bid = {0, 1, 0};
    const std::vector<float> D = {1, 1, 0,
                                  0, 0, 1};
    CHECK(!vc_batch_conditions(D.data(), 2, 3, bid, 2, cond));
    CHECK(cond.empty());
  }
  // D not one-hot: a fractional entry, a cell in two conditions, a cell in none
  {
    const std::vector<int> bid = {0, 1};
    const std::vector<float> frac = {0.5f, 1, 0.5f, 0}, both = {1, 1, 1, 0}, none = {0, 1, 0, 0};
    for (const auto* D : {&frac, &both, &none}) {
      CHECK(!vc_batch_conditions(D->data(), 2, 2, bid, 2, cond));
      CHECK(cond.empty());
    }
    CHECK(!vc_batch_conditions(frac.data(), 0, 2, bid, 2, cond));      // no condition rows at all
  }
  // a batch with no cells on this rank: condition 0
  {
    const std::vector<int> bid = {0, 2, 2};
    const std::vector<float> D = {0, 0, 0,
                                  0, 1, 1,
                                  1, 0, 0};
    CHECK(vc_batch_conditions(D.data(), 3, 3, bid, 3, cond));
    CHECK((cond == std::vector<int>{2, 0, 1}));
  }
}

// Dense tail-count tables (vc_build_dense_hist) and their per-quarter largest counts (vc_hist_quarter_rows) against a brute-force
// recount, at the level limits of the device evaluators (255 / 256 / 257: the first 256 levels are prefetched; 639 / 640 / 641: the
// second loop; 2047: the last dense bin).  kmax[g] = the largest count of gene g (0: an all-zero gene); `top` cells sit at it.
static void dense_hist_case(const std::vector<int>& kmax, int Nc, int top, unsigned seed) {
  std::mt19937 rng(seed);
  const int Ng = (int)kmax.size(), Ng_pad = (Ng + 63) / 64 * 64, nblk = Ng_pad / 64;
  std::vector<int> M((size_t)Ng * Nc, 0);
  std::vector<unsigned> tab((size_t)Ng * VC_HIST_CAP, 0u);
  for (int g = 0; g < Ng; ++g) {
    const int K = kmax[(size_t)g];
    CHECK(K >= 0 && K < VC_HIST_CAP && top <= Nc);
    for (int c = 0; c < Nc && K > 0; ++c) {
      int v = c < top ? K : (int)(rng() % (unsigned)K);             // below the top level: anything in [0, K)
      if (c >= top && rng() % 3 == 0) v = 0;
      M[(size_t)g * Nc + c] = v;
      if (v) tab[(size_t)g * VC_HIST_CAP + v]++;
    }
  }
  std::vector<float> HC;
  std::vector<int> off, rows;
  vc_build_dense_hist(tab.data(), Ng, Ng_pad, HC, off, rows);
  CHECK((int)off.size() == nblk && (int)rows.size() == nblk);
  size_t nrows = 0;
  for (int gb = 0; gb < nblk; ++gb) {
    int want = 0;
    for (int g = gb * 64; g < std::min(Ng, gb * 64 + 64); ++g) want = std::max(want, kmax[(size_t)g]);
    CHECK(rows[(size_t)gb] == want);
    CHECK(off[(size_t)gb] == (int)nrows);
    nrows += (size_t)rows[(size_t)gb];
  }
  CHECK(HC.size() == nrows * 64);
  const double rs[] = {1e-4, 1e-2, 0.37, 1.0, 8.0, 123.4, 1e4};
  for (int gb = 0; gb < nblk; ++gb)
    for (int l = 0; l < 64; ++l) {
      const int g = gb * 64 + l;
      for (int j = 0; j < rows[(size_t)gb]; ++j) {
        unsigned want = 0;                                           // C_j = cells whose count is > j
        for (int c = 0; c < Nc && g < Ng; ++c) want += M[(size_t)g * Nc + c] > j;
        CHECK(HC[((size_t)off[(size_t)gb] + j) * 64 + l] == (float)want);
      }
      if (g >= Ng) continue;
      // sum_j C_j log(r + j) = sum_k cnt_k (lgamma(r + k) - lgamma(r)), and the digamma twin sum_j C_j / (r + j), in double
      for (double r : rs) {
        double tl = 0, ll = 0, ts = 0;
        for (int j = 0; j < rows[(size_t)gb]; ++j) {
          const double cj = HC[((size_t)off[(size_t)gb] + j) * 64 + l];
          tl += cj * std::log(r + j);
          ts += std::fabs(cj * std::log(r + j));
        }
        for (int k = 1; k < VC_HIST_CAP; ++k)
          if (tab[(size_t)g * VC_HIST_CAP + k]) ll += (double)tab[(size_t)g * VC_HIST_CAP + k] * (std::lgamma(r + k) - std::lgamma(r));
        CHECK(std::fabs(tl - ll) <= 1e-11 * (1.0 + ts));
      }
    }
  // the quarter blocks: each quarter to its own genes' largest count; the blocks past 256 levels are split
  std::vector<int> rows_q, split;
  vc_hist_quarter_rows(HC, off, rows, 256, rows_q, split);
  CHECK(rows_q.size() == rows.size() * 4);
  std::vector<int> want_split;
  for (int gb = 0; gb < nblk; ++gb) {
    int mx = 0;
    for (int qd = 0; qd < 4; ++qd) {
      int want = 0;
      for (int g = gb * 64 + 16 * qd; g < std::min(Ng, gb * 64 + 16 * qd + 16); ++g) want = std::max(want, kmax[(size_t)g]);
      CHECK(rows_q[(size_t)gb * 4 + qd] == want);
      mx = std::max(mx, want);
    }
    CHECK(mx == rows[(size_t)gb]);
    if (rows[(size_t)gb] > 256) want_split.push_back(gb);
  }
  CHECK(split == want_split);
}

static void dense_hist_cases() {
  const int lv[] = {0, 1, 255, 256, 257, 639, 640, 641, 2047};
  // one largest count per block (all 64 genes at it, or one gene at it beside small genes), Ng not a multiple of 64
  for (int K : lv) {
    dense_hist_case(std::vector<int>(64, K), 24, 20, 10 + K);
    std::vector<int> km(100, K > 0 ? std::min(K, 3) : 0);
    km[37] = K;
    km[99] = K;                                                      // the last gene of a ragged block
    dense_hist_case(km, 30, 20, 20 + K);
  }
  // 200 genes: every level limit in block 0, an all-zero gene, one all-zero quarter next to a quarter past 640 levels in block 1,
  // block 2 entirely zero, a ragged block 3
  std::vector<int> km(200, 0);
  for (int i = 0; i < 9; ++i) km[(size_t)i] = lv[i];
  for (int g = 9; g < 64; ++g) km[(size_t)g] = 1 + g % 7;
  for (int g = 64; g < 80; ++g) km[(size_t)g] = 0;                   // quarter 0 of block 1: zero
  for (int g = 80; g < 96; ++g) km[(size_t)g] = 640 + (g & 3);        // quarter 1: 640 .. 643
  for (int g = 96; g < 128; ++g) km[(size_t)g] = 5;
  for (int g = 192; g < 200; ++g) km[(size_t)g] = g == 199 ? 2047 : 2;
  dense_hist_case(km, 40, 20, 7);
  dense_hist_case(std::vector<int>(1, 0), 5, 0, 8);                 // one all-zero gene
  dense_hist_case(std::vector<int>(130, 0), 5, 0, 9);               // every block empty
  dense_hist_case(std::vector<int>(1, 2047), 1, 1, 10);             // a single cell
}

int main() {
  dense_hist_cases();
  condition_cases();
  {
    std::mt19937 rng(5);
    for (int it = 0; it < 120; ++it)
      batch_case(1 + (long long)(rng() % 60000), 1 + (int)(rng() % 13), 1 + (int)(rng() % 8), (it % 4 == 0) ? 1 + (int)(rng() % 300) : 256,
                 1 + (int)(rng() % 4), it % 2 == 1, 100 + it);
    batch_case(50000, 2, 4, 256, 2, false, 1);
    batch_case(50000, 8, 4, 256, 2, true, 2);
    batch_case(23, 2, 1, 256, 2, false, 3);
    batch_case(5, 5, 1, 256, 3, true, 4);
  }
  {
    const double half[4] = {1.0, 0.5, 0.25, 0.125}, flat[4] = {1, 1, 1, 1}, odd[4] = {0.5, 0.3, 0.2, 0.2}, steep[4] = {0.85, 0.15, 0.15, 0.15};
    std::mt19937 rng(11);
    for (int it = 0; it < 400; ++it) {
      const long long Nc = 1 + (long long)(rng() % 200000) * (it % 7 == 0 ? 13 : 1);
      const int nGB = 1 + (int)(rng() % 9), n_cu = (it % 5 == 0) ? 1 + (int)(rng() % 300) : 256, bpc = 1 + (int)(rng() % 5);
      const double* sh[] = {half, flat, odd, steep, nullptr};
      tiling_case(Nc, nGB, n_cu, bpc, sh[rng() % 5], (it % 3 == 0) ? 1 : 12, (it % 11 == 0) ? 1 + (long long)(rng() % 300) : 0);
    }
    tiling_case(50000, 4, 256, 2, half, 12, 0);
    tiling_case(50000, 4, 256, 3, half, 12, 0);
    tiling_case(9000, 3, 256, 2, half, 12, 0);
    tiling_case(1, 1, 256, 2, half, 12, 0);
    const VcTiling t = vc_tile_cells(50000, 4, 256, 2, 4, 0, half, 12);
    CHECK(t.n_chunks == 128 && t.pass_cw[0] == 131 && t.pass_cw[1] == 66);
  }
  one_case(7, 33, false, false, 1);
  one_case(7, 33, true, true, 2);
  one_case(64, 301, false, true, 3);
  one_case(1, 1, true, false, 4);
  one_case(130, 77, true, true, 5);
  // invalid values are flagged, never converted to int (UB) or used as map keys
  {
    std::vector<float> M = {1.f, std::numeric_limits<float>::quiet_NaN(), 3.f, -2.f, std::numeric_limits<float>::infinity(), 1e30f};
    std::vector<int> ptr;
    std::vector<float> val, cnt;
    bool bad = false;
    vc_build_hist_host(M.data(), 3, 1, 2, 3, ptr, val, cnt, &bad);
    CHECK(bad);
    CHECK(!vc_count_ok(M[1]) && !vc_count_ok(M[3]) && !vc_count_ok(M[4]) && vc_count_ok(M[5]) && !vc_count_dense(M[5]));
  }
  if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
  std::printf("host logic ok\n");
  return 0;
}
