// check_live_rate.cpp — the host arithmetic of csrc/tfp_live_rate.hpp, stand-alone: the settled count
// against the definition, the carry bound, the streaming routine against the whole-clip map under random
// splits of the input, the zero flush, the tile table and the capacity refusal. Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all and run on the CPU: any finding aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfp_live_rate.hpp"

namespace tfp {
// (tfp_resample.cpp's cache is not linked here; the checks build their tables themselves)
std::shared_ptr<const ResampleTable> resample_table(int32_t, int32_t, bool*) { return nullptr; }
}  // namespace tfp

using namespace tfp;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      return 1;                                                     \
    }                                                               \
  } while (0)

static uint32_t rng_state = 2468u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// The first n samples of the whole-clip map of x.
static std::vector<int16_t> clip_head(const ResampleTable& t, const std::vector<int16_t>& x, int64_t n) {
  std::vector<int16_t> y((size_t)resample_count(t.plan, (int64_t)x.size()));
  resample_clip(t, x.data(), (int64_t)x.size(), y.data());
  if ((int64_t)y.size() < n) std::abort();  // (more settled than the clip has outputs: a finding)
  y.resize((size_t)n);
  return y;
}

int main() {
  const int32_t pairs[][2] = {{16000, 8000}, {48000, 8000}, {8000, 16000}, {44100, 8000},
                              {11025, 8000}, {44100, 48000}, {8001, 8000}};
  const int64_t lags[] = {48, 144, 24, 133, -1, -1, -1};  // the header's table
  int pi = 0;
  for (const auto& pr : pairs) {
    ResampleTable t;
    bool bad = false;
    CHECK(resample_plan(pr[0], pr[1], &t.plan, &bad) && resample_build(t.plan, &t.taps));
    const ResamplePlan& P = t.plan;
    const int64_t k_hi = live_rate_lag(P), nt = P.ntaps;
    CHECK(k_hi == (int64_t)P.k_lo + P.ntaps - 1 && k_hi >= 0);
    if (lags[pi] >= 0) CHECK(k_hi == lags[pi]);
    pi++;
    CHECK(live_rate_supported(P));
    const int32_t tile = live_rate_tile(P);
    CHECK(tile >= 2 && tile <= kRsTile && live_rate_span(P, tile) <= kLiveRateSpanMax);
    CHECK(tile == kRsTile || live_rate_span(P, tile + 1) > kLiveRateSpanMax);

    // the settled count by the definition, and the carry bound, at every S_in up to 3 ntaps
    for (int64_t s_in = 0; s_in <= 3 * nt + 7; s_in++) {
      int64_t n = 0;
      while ((n * P.M) / P.L + k_hi <= s_in - 1) n++;
      CHECK(live_rate_settled(P, s_in) == n);
      if (s_in <= k_hi) CHECK(n == 0);
      CHECK((n * P.M) / P.L + P.k_lo >= s_in - (nt - 1));  // the first unsettled output's first tap
      LiveRateStep st;
      CHECK(live_rate_step(P, s_in, 5, &st));
      CHECK(st.n_old == n && st.s_in_new == s_in + 5 && st.carry_lo == s_in + 5 - (nt - 1));
      CHECK(st.n_old + st.n_new == live_rate_settled(P, s_in + 5));
    }

    // streaming against the whole clip: noise and full-scale rails, random splits
    for (int kind = 0; kind < 2; kind++) {
      const int64_t n_in = 3 * nt + 11;
      std::vector<int16_t> x((size_t)n_in);
      for (int64_t i = 0; i < n_in; i++)
        x[(size_t)i] = kind ? (int16_t)(((i / P.M) & 1) ? -32767 : 32767) : (int16_t)(rnd() & 0xffff);
      if (!kind) x[0] = -32768, x[1] = 32767, x[(size_t)n_in - 1] = -32768;
      for (int trial = 0; trial < 12; trial++) {
        LiveRateHost st;
        std::vector<int16_t> hist;
        if (trial & 1) {  // a call before this one that ended on rails: reset, nothing may leak
          std::vector<int16_t> loud((size_t)(2 * nt), (int16_t)32767);
          CHECK(live_rate_push_host(t, &st, loud.data(), (int64_t)loud.size(), INT64_MAX, &hist) == 0);
          st.reset();
          hist.clear();
        }
        const int64_t forced[] = {0, 1, nt - 1, nt + 1, 0, 1};
        int64_t at = 0;
        for (int step = 0; at < n_in; step++) {
          int64_t n = step < 6 ? forced[(step + trial) % 6] : (int64_t)(rnd() % (uint32_t)(nt + 3));
          if (n > n_in - at) n = n_in - at;
          std::vector<int16_t> tick(x.begin() + at, x.begin() + at + n);  // exactly n samples: a read past it is a finding
          const int parity = st.parity;
          CHECK(live_rate_push_host(t, &st, tick.data(), n, INT64_MAX, &hist) == 0);
          CHECK(st.parity == (n > 0 ? 1 - parity : parity));  // an idle channel keeps its parity
          at += n;
          CHECK(st.s_in == at);
          CHECK((int64_t)hist.size() == live_rate_settled(P, at));
          std::vector<int16_t> sofar(x.begin(), x.begin() + at);
          CHECK(hist == clip_head(t, sofar, (int64_t)hist.size()));
        }
        // every continuation: the settled samples are the head of the whole clip's map too
        CHECK(hist == clip_head(t, x, (int64_t)hist.size()));
        // the zero flush
        std::vector<int16_t> zeros((size_t)k_hi, 0);
        CHECK(live_rate_push_host(t, &st, zeros.data(), k_hi, INT64_MAX, &hist) == 0);
        CHECK((int64_t)hist.size() == resample_count(P, n_in));
        CHECK(hist == clip_head(t, x, (int64_t)hist.size()));
      }
    }

    // the capacity refusal leaves the state untouched
    {
      LiveRateHost st;
      std::vector<int16_t> hist, x((size_t)(2 * nt + 40), (int16_t)1234);
      CHECK(live_rate_push_host(t, &st, x.data(), nt + 20, INT64_MAX, &hist) == 0);
      const LiveRateHost before = st;
      const std::vector<int16_t> hist_before = hist;
      const int64_t cap = live_rate_settled(P, st.s_in + nt + 20) - 1;
      CHECK(cap >= (int64_t)hist.size());
      CHECK(live_rate_push_host(t, &st, x.data() + nt + 20, nt + 20, cap, &hist) == 1);
      CHECK(st.s_in == before.s_in && st.parity == before.parity && st.carry[0] == before.carry[0] &&
            st.carry[1] == before.carry[1] && hist == hist_before);
      CHECK(live_rate_push_host(t, &st, x.data() + nt + 20, nt + 20, cap + 1, &hist) == 0);
      CHECK(hist == clip_head(t, x, (int64_t)hist.size()) && (int64_t)hist.size() == cap + 1);
    }

    // the tile table covers each channel's new outputs exactly once, and names each moving channel once
    {
      const int32_t news[] = {0, 1, tile - 1, tile, tile + 1, 2 * tile + 1, 0, 3};
      const int32_t ins[] = {0, 4, 9, 9, 9, 9, 2, 0};  // (n_new > 0 with n_in = 0 does not occur; the table does not care)
      std::vector<LiveRateChan> chan;
      for (int i = 0; i < 8; i++) chan.push_back(LiveRateChan{0, 100 + i, ins[i], news[i], i & 1, 0});
      std::vector<int32_t> toff, tclip;
      const int32_t ntiles = live_rate_tiles(chan.data(), 8, tile, &toff, &tclip);
      CHECK((int32_t)toff.size() == 9 && toff[0] == 0 && toff[8] == ntiles);
      std::vector<std::vector<int>> seen(8);
      for (int i = 0; i < 8; i++) seen[(size_t)i].assign((size_t)news[i], 0);
      for (int32_t b = 0; b < ntiles; b++) {
        const int32_t c = tclip.at((size_t)b);
        CHECK(c >= 0 && c < 8 && b >= toff[(size_t)c] && b < toff[(size_t)c + 1]);
        const int64_t j0 = (int64_t)(b - toff[(size_t)c]) * tile, j1 = j0 + tile < news[c] ? j0 + tile : news[c];
        CHECK(j0 < j1);
        for (int64_t j = j0; j < j1; j++) seen[(size_t)c].at((size_t)j)++;
      }
      for (int i = 0; i < 8; i++)
        for (int v : seen[(size_t)i]) CHECK(v == 1);
      std::vector<int32_t> moved(tclip.begin() + ntiles, tclip.end());
      CHECK(moved == (std::vector<int32_t>{1, 2, 3, 4, 5, 6}));
    }
  }
  // refusals: a filter past the staged span, with a table inside 2^20 entries
  {
    ResamplePlan P;
    bool bad = false;
    CHECK(resample_plan(5600000, 8000, &P, &bad) && !live_rate_supported(P));
    CHECK(resample_plan(96000, 8000, &P, &bad) && live_rate_supported(P));
    CHECK(!resample_plan(7999, 44100, &P, &bad) && !bad);
  }
  std::printf("OK\n");
  return 0;
}
