// Self-test of the scheduler's match_limit (csrc/runtime/runtime_core.h): the number of leading prompt tokens a request
// may be served from cached blocks.  A stand-alone program, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_prompt_logprobs_cpu.py (host code only).  Exits non-zero on the first broken expectation.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../runtime/runtime_core.h"

#define REQUIRE(c)                                                       \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static void drain(Scheduler& s) {
  s.take_copies();
  s.copies_done();
}

// cached tokens a request with `limit` finds for `toks`; the request is finished again
static int hit(Scheduler& s, long long id, const std::vector<int>& toks, int limit, bool with_limit = true) {
  if (with_limit)
    s.add(id, (int)toks.size(), 4, toks, true, limit);
  else
    s.add(id, (int)toks.size(), 4, toks, true);
  const auto adm = s.admit();
  REQUIRE(adm.size() == 1 && adm[0] == id);
  const int n = s.cached_tokens(id);
  drain(s);
  s.finish(id);
  return n;
}

int main() {
  std::mt19937 rng(12345);
  long long id = 1;
  for (int round = 0; round < 200; ++round) {
    const int bs = 1 << (1 + rng() % 4);           // 2 .. 16
    const int cow = 1 + rng() % bs;                // 1 .. bs
    const int n = bs + 1 + rng() % (6 * bs);       // at least one full block
    std::vector<int> toks(n);
    for (int i = 0; i < n; ++i) toks[i] = 100 + (i * 7 + round) % 9973;
    Scheduler s(256, bs, 4, 1 << 20, 64, 8, true, cow);
    s.add(id, n, 4, toks, true);
    REQUIRE(s.admit().size() == 1 && s.cached_tokens(id) == 0);
    s.publish(id);
    s.finish(id);
    ++id;
    const int full = n / bs * bs;  // tokens in published blocks
    // what a cap allows: whole cached blocks under it, then the next published block's first tokens (the fork), up to
    // the cap and if worth a copy
    auto expect = [&](int cap) {
      const int blocks = std::min(cap, full) / bs * bs;
      int fork = std::min({bs - 1, cap - blocks, std::max(0, full - blocks)});
      if (fork < cow) fork = 0;
      return blocks + fork;
    };
    const int today = hit(s, id++, toks, 0, false);  // the default: at least the last token is computed
    REQUIRE(today == expect(n - 1));
    REQUIRE(hit(s, id++, toks, -1) == today);
    REQUIRE(hit(s, id++, toks, n - 1) == today);
    REQUIRE(hit(s, id++, toks, n + 17) == today);
    for (int limit = 0; limit < n; ++limit) {
      const int got = hit(s, id++, toks, limit);
      REQUIRE(got <= limit);
      REQUIRE(got == expect(limit));
    }
    // a preempted request takes the limit of its resumed prompt
    s.add(id, n, 8, toks, true, 0);
    REQUIRE(s.admit().size() == 1 && s.cached_tokens(id) == 0);
    drain(s);
    std::vector<int> longer(toks);
    longer.push_back(3);
    longer.push_back(4);
    const int lim = (int)(rng() % n);
    s.preempt(id, (int)longer.size(), 4, longer, lim);
    REQUIRE(s.admit().size() == 1 && s.cached_tokens(id) <= lim);
    drain(s);
    s.preempt(id, (int)longer.size(), 4, longer);  // no limit given: the default rule again
    REQUIRE(s.admit().size() == 1 && s.cached_tokens(id) >= today);
    drain(s);
    s.finish(id++);
  }
  std::printf("match_limit selftest ok\n");
  return 0;
}
