// Core of the native host runtime (no Python dependency): the paged-KV block allocator, the
// continuous-batching scheduler and the UTF-8 edit distance.  runtime.cpp binds it as `_lsa_runtime`;
// csrc/tests/runtime_selftest.cpp drives it under AddressSanitizer + UBSan (tests/test_native_sanitizers.py).
#pragma once
#include <algorithm>
#include <deque>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

// ------------------------------------------------------------------------------------------ utf-8
inline std::u32string utf8_to_u32(const std::string& s) {
  std::u32string out;
  out.reserve(s.size());
  size_t i = 0;
  while (i < s.size()) {
    unsigned char c = s[i];
    char32_t cp;
    int n;
    if (c < 0x80) { cp = c; n = 1; }
    else if ((c >> 5) == 0x6) { cp = c & 0x1f; n = 2; }
    else if ((c >> 4) == 0xe) { cp = c & 0x0f; n = 3; }
    else { cp = c & 0x07; n = 4; }
    for (int k = 1; k < n && i + k < s.size(); ++k) cp = (cp << 6) | (s[i + k] & 0x3f);
    out.push_back(cp);
    i += n;
  }
  return out;
}

inline int levenshtein_u32(const std::u32string& a, const std::u32string& b) {
  const std::u32string& s = a.size() < b.size() ? b : a;  // longer
  const std::u32string& t = a.size() < b.size() ? a : b;  // shorter: O(|t|) memory
  std::vector<int> prev(t.size() + 1), cur(t.size() + 1);
  for (size_t j = 0; j <= t.size(); ++j) prev[j] = (int)j;
  for (size_t i = 1; i <= s.size(); ++i) {
    cur[0] = (int)i;
    for (size_t j = 1; j <= t.size(); ++j) {
      const int sub = prev[j - 1] + (s[i - 1] == t[j - 1] ? 0 : 1);
      cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, sub});
    }
    std::swap(prev, cur);
  }
  return prev[t.size()];
}

inline int levenshtein(const std::string& a, const std::string& b) { return levenshtein_u32(utf8_to_u32(a), utf8_to_u32(b)); }

// ------------------------------------------------------------------------------------- allocator
class BlockAllocator {
 public:
  BlockAllocator(int num_blocks, int block_size) : num_blocks_(num_blocks), block_size_(block_size) {
    if (num_blocks < 2) throw std::invalid_argument("need at least 2 KV blocks (block 0 is scratch)");
    free_.reserve(num_blocks);
    for (int b = num_blocks - 1; b >= 1; --b) free_.push_back(b);
    owned_.assign(num_blocks, 0);
  }
  int blocks_for(int tokens) const { return (tokens + block_size_ - 1) / block_size_; }
  bool can_alloc(int n) const { return (int)free_.size() >= n; }
  std::vector<int> alloc(int n) {
    if (!can_alloc(n)) throw std::runtime_error("KV cache exhausted");
    if (n < 0) throw std::invalid_argument("negative block count");
    std::vector<int> out(free_.end() - n, free_.end());
    free_.resize(free_.size() - n);
    std::reverse(out.begin(), out.end());
    for (int b : out) owned_[b] = 1;
    return out;
  }
  void release(const std::vector<int>& blocks) {
    for (int b : blocks)  // validate everything first: a bad list releases nothing
      if (b <= 0 || b >= num_blocks_ || !owned_[b]) throw std::invalid_argument("bad or already-free block id");
    std::vector<int> sorted(blocks);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      throw std::invalid_argument("block listed twice");
    for (int b : blocks) {
      owned_[b] = 0;
      free_.push_back(b);
    }
  }
  int num_free() const { return (int)free_.size(); }
  int num_blocks() const { return num_blocks_; }
  int block_size() const { return block_size_; }

 private:
  int num_blocks_, block_size_;
  std::vector<int> free_;
  std::vector<unsigned char> owned_;  // 1 while a block is handed out (double-free / foreign-id guard)
};

// ------------------------------------------------------------------------------------- scheduler
// KV reservation is lazy: admission reserves the prompt plus at most `reserve_tokens` generated tokens (one 64-token
// block by default; < 0 = the whole prompt + max_new up front, the pre-round-4 behaviour), and the engine grows a
// running request's table before each decode run (grow) as its context crosses block boundaries.  When the arena is
// exhausted the engine preempts (preempt): the request's blocks and slot are released and it is re-queued at the
// FRONT of the waiting queue with its generated tokens folded into its prompt (recompute on re-admission).  Without
// this, Ollama's generate-until-EOS default (max_new = the whole remaining window) pinned a full-window KV reservation
// per request for a ~30-token SQL answer.
struct Req {
  long long id;
  int prompt_len;
  int max_new;
  int slot = -1;
  long long admit_seq = -1;  // admission order (preemption picks the youngest)
  std::vector<int> blocks;
  // prefix cache (all empty / zero when it is off or the request opted out)
  std::vector<int> tokens;  // the prompt's token ids
  bool cacheable = false;
  bool published = false;
  int cached = 0;           // prompt tokens whose KV the request found in the cache at admission
  int match_limit = -1;     // leading tokens that may be served from cached blocks; < 0 = prompt_len - 1
  std::vector<int> nodes;   // index nodes behind blocks[0 .. nodes.size()): the shared head of the table
};

// Prefix cache (prefix_cache = true; off by default, and then nothing below runs).  The index is a trie of FULL
// blocks of prompt tokens: a node stands for one KV block whose block_size rows hold the keys / values of its
// token ids in the context of its ancestors' token ids.  A request's table is [shared blocks..., private blocks...]:
// the shared head are nodes it holds a reference on, found at admission or published by itself.  A node nobody
// references stays cached and counts as allocatable; such nodes are evicted leaf-first in least-recently-used
// order when the free list runs short.  A holder of a node holds every ancestor too, so the unreferenced nodes
// are closed under "descendant of" and every one of them can be reached by leaf-first eviction.
//
// Reuse is token-granular: past the last matched full block, admission looks among that node's children for the
// longest common prefix p with the prompt's next tokens and, if p >= cow_min_tokens, forks it: the request gets a
// fresh private block and a pending copy (src block, dst block) that the engine runs before the prefill
// (take_copies / copies_done; the source and its ancestors stay pinned in between).
//
// Safety invariant: no kernel writes a block that the index holds.  Published blocks lie entirely below their
// owner's prompt_len (publish inserts only full prompt blocks, after the prompt's last prefill chunk is launched);
// every later write of the owner is at positions >= prompt_len (decode appends, the stale rows of a verify step, a
// finished row rewriting its last T positions; a row finished by its prefill token is parked at prompt_len for
// this, ModelRunner.park_past_prompt).  A sharer writes only at positions >= its cached_tokens, which lie
// in its private blocks (the forked block is private).  Idle rows write block 0, which is never handed out.
//
// Known limit: requests admitted by the same admit() call do not share with each other (the first one publishes
// only after its prefill).
struct PrefixNode {
  int parent = -1;
  std::vector<int> toks;      // block_size token ids
  int block = -1;
  int ref = 0;                // running requests (and pending copies) that hold the node
  std::vector<int> children;  // insertion order; child count = children.size()
  long long tick = 0;         // last use
  bool live = false;
};

class Scheduler {
 public:
  Scheduler(int num_blocks, int block_size, int max_slots, int max_prefill_tokens, int max_blocks_per_seq,
            int reserve_tokens = 64, bool prefix_cache = false, int cow_min_tokens = kCowMinTokens)
      : alloc_(num_blocks, block_size), max_slots_(max_slots), max_prefill_tokens_(max_prefill_tokens),
        max_blocks_per_seq_(max_blocks_per_seq), reserve_tokens_(reserve_tokens), slots_(max_slots, -1),
        prefix_cache_(prefix_cache), cow_min_(std::max(1, cow_min_tokens)), nodes_(1) {
    nodes_[0].live = true;  // the root: the empty prefix, never evicted
  }

  // Smallest common prefix with a cached block that is worth forking it (copy the block, prefill the rest).
  // Rule: the smallest p of the sweep 8 / 16 / 32 / 48 whose saved time to first token is at least twice the copy's
  // device time on both served models (scripts/bench_prefix_cache.py, profiles/prefix_cache/cow_sweep_mi355x.jsonl):
  //   7B  copy 21.6 us; saved (suffix 32 + p against 32, behind 256 cached tokens) 921 / 1304 / 2057 / 1566 us
  //   3B  copy 17.3 us; saved 609 / 747 / 1055 / 1420 us
  // p = 8 saves 43x (7B) and 35x (3B) the copy, so the default is 8.
  static constexpr int kCowMinTokens = 8;

  // tokens: the prompt's token ids, required (and length-checked) when the prefix cache is on and the request is
  // cacheable; ignored otherwise.  match_limit: the number of leading prompt tokens that may be served from cached
  // blocks (full blocks and the fork alike); < 0 = prompt_len - 1, the rule that at least the last prompt token is
  // computed.  A request whose prompt rows from some position on must be computed (prompt-token logprobs) passes less.
  void add(long long id, int prompt_len, int max_new, const std::vector<int>& tokens = {}, bool cacheable = true,
           int match_limit = -1) {
    if (reqs_.count(id)) throw std::invalid_argument("duplicate request id");
    if (prompt_len < 1 || max_new < 1) throw std::invalid_argument("empty prompt or max_new < 1");
    const int need = alloc_.blocks_for(prompt_len + max_new);
    if (need > max_blocks_per_seq_) throw std::invalid_argument("request exceeds max model length");
    if (need > alloc_.num_blocks() - 1) throw std::invalid_argument("request larger than the whole KV cache");
    const bool cache = prefix_cache_ && cacheable;
    if (cache && (int)tokens.size() != prompt_len) throw std::invalid_argument("tokens must hold prompt_len ids");
    Req& r = reqs_[id] = Req{id, prompt_len, max_new};
    if (cache) {
      r.tokens = tokens;
      r.cacheable = true;
      r.match_limit = match_limit;
    }
    waiting_.push_back(id);
  }

  // blocks reserved when a request is admitted
  int admit_blocks(const Req& r) const {
    const int gen = reserve_tokens_ < 0 ? r.max_new : std::min(r.max_new, reserve_tokens_);
    return alloc_.blocks_for(r.prompt_len + gen);
  }

  // Admit waiting requests (FCFS) while a slot, the prefill budget and KV blocks allow.
  // Returns the ids admitted this step (to be prefilled) — each now owns a slot and its blocks.
  std::vector<long long> admit() {
    std::vector<long long> out;
    int budget = max_prefill_tokens_;
    while (!waiting_.empty()) {
      Req& r = reqs_.at(waiting_.front());
      // the cache can change while a request waits, so it is matched here, not in add()
      const Match m = r.cacheable ? match(r) : Match{};
      const int cached = (int)m.chain.size() * alloc_.block_size() + m.p;
      if (!out.empty() && r.prompt_len - cached > budget) break;  // always admit at least one if it fits
      const int need = admit_blocks(r) - (int)m.chain.size();
      // hold the matched nodes and the fork's source first: they must not count as allocatable below
      for (int n : m.chain) ref_node(n);
      if (m.src >= 0) ref_chain(m.src);
      int slot = -1;
      for (int s = 0; s < max_slots_; ++s)
        if (slots_[s] < 0) { slot = s; break; }
      if (available() < need || slot < 0) {
        for (int n : m.chain) unref_node(n);
        if (m.src >= 0) unref_chain(m.src);
        break;
      }
      if (r.cacheable) ++clock_;
      r.nodes = m.chain;
      r.blocks.clear();
      for (int n : m.chain) {
        nodes_[n].tick = clock_;
        r.blocks.push_back(nodes_[n].block);
      }
      const std::vector<int> priv = take(need);
      r.blocks.insert(r.blocks.end(), priv.begin(), priv.end());
      if (m.src >= 0) {  // the pin (held above) stays until copies_done()
        nodes_[m.src].tick = clock_;
        copies_.emplace_back(nodes_[m.src].block, priv[0]);
        pins_.push_back(m.src);
      }
      r.cached = cached;
      r.slot = slot;
      r.admit_seq = ++admit_counter_;
      slots_[slot] = r.id;
      budget -= r.prompt_len - cached;
      out.push_back(r.id);
      waiting_.pop_front();
    }
    return out;
  }

  // Make a running request own the blocks for its first `tokens` cache positions (capped at prompt + max_new).
  // Returns the number of blocks added (0 if it already had them), or -1 when the arena cannot supply them
  // (nothing is allocated then).
  int grow(long long id, int tokens) {
    Req& r = reqs_.at(id);
    if (r.slot < 0) throw std::invalid_argument("grow: request is not running");
    const int want = std::min(alloc_.blocks_for(std::min(tokens, r.prompt_len + r.max_new)), max_blocks_per_seq_);
    const int add = want - (int)r.blocks.size();
    if (add <= 0) return 0;
    if (available() < add) return -1;
    const std::vector<int> nb = take(add);
    r.blocks.insert(r.blocks.end(), nb.begin(), nb.end());
    return add;
  }

  // Release a running request's slot and blocks and put it back at the front of the waiting queue with a new
  // (prompt, max_new): the engine folds the tokens generated so far into the prompt and re-prefills them.
  // With the prefix cache on, tokens are the resumed prompt's ids (as in add): the request can then hit its own
  // earlier blocks on re-admission if they survived.
  // match_limit: as in add, for the resumed prompt.
  void preempt(long long id, int prompt_len, int max_new, const std::vector<int>& tokens = {}, int match_limit = -1) {
    Req& r = reqs_.at(id);
    if (r.slot < 0) throw std::invalid_argument("preempt: request is not running");
    if (prompt_len < 1 || max_new < 1 || alloc_.blocks_for(prompt_len + max_new) > max_blocks_per_seq_)
      throw std::invalid_argument("preempt: bad resumed lengths");
    if (r.cacheable && (int)tokens.size() != prompt_len) throw std::invalid_argument("tokens must hold prompt_len ids");
    slots_[r.slot] = -1;
    r.slot = -1;
    r.admit_seq = -1;
    release_blocks(r);
    r.prompt_len = prompt_len;
    r.max_new = max_new;
    if (r.cacheable) r.tokens = tokens;
    r.match_limit = match_limit;
    waiting_.push_front(id);
  }

  // running requests, youngest admission first (the engine's preemption order)
  std::vector<long long> youngest_first() const {
    std::vector<std::pair<long long, long long>> v;
    for (long long s : slots_)
      if (s >= 0) v.emplace_back(-reqs_.at(s).admit_seq, s);
    std::sort(v.begin(), v.end());
    std::vector<long long> out;
    for (auto& p : v) out.push_back(p.second);
    return out;
  }

  void finish(long long id) {
    auto it = reqs_.find(id);
    if (it == reqs_.end()) return;
    Req& r = it->second;
    if (r.slot >= 0) slots_[r.slot] = -1;
    release_blocks(r);
    waiting_.erase(std::remove(waiting_.begin(), waiting_.end(), id), waiting_.end());
    reqs_.erase(it);
  }

  // ---------------------------------------------------------------------------------- context shift
  // Plan of one context shift (shift): the KV moves (src block, dst block, row_lo, row_hi, delta) for ops.kv_shift
  // and the request's new block table.  ok = false: refused, nothing changed.
  struct ShiftPlan {
    bool ok = false;
    std::vector<std::vector<int>> moves;
    std::vector<int> table;
  };

  // Drop the tokens at positions [keep, keep + discard) of a running request's cache, discard a positive multiple of
  // the block size: the token at old position p >= keep + discard moves to p - discard, i.e. down discard / bs table
  // entries in the same row of its block, its K rotated by -discard.  For each new logical block j >= keep / bs the
  // rows come from old logical block j + discard / bs -- except rows below keep % bs of block keep / bs, which are
  // copied from old block keep / bs (delta 0).  The destination is the source block itself when the request owns it
  // privately (the rotation is then in place), else a fresh block: a block the index holds is never written (the
  // invariant above).  Blocks below keep / bs stay as they are and may stay shared; from keep / bs on every block of
  // the new table is private.  Every other old block is released: private ones to the free list, index nodes
  // unreferenced -- a suffix of the request's chain, so a holder still holds every ancestor.  Fresh blocks are taken
  // first (evicting unreferenced cached blocks as grow does); if the arena cannot supply them the plan is refused and
  // nothing changes.  The released blocks are still read by the planned moves, so they stay out of the free list,
  // and the nodes referenced, until shift_done(), which the engine calls once the moves are enqueued.
  ShiftPlan shift(long long id, int keep, int discard) {
    Req& r = reqs_.at(id);
    const int bs = alloc_.block_size(), nb = (int)r.blocks.size();
    if (r.slot < 0) throw std::invalid_argument("shift: request is not running");
    if (keep < 0 || discard <= 0 || discard % bs) throw std::invalid_argument("shift: bad keep or discard");
    const int k0 = keep / bs, rem = keep % bs, m = discard / bs, shared = (int)r.nodes.size();
    if (k0 + m >= nb) throw std::invalid_argument("shift: nothing left behind the discarded tokens");
    ShiftPlan plan;
    int fresh = 0;
    for (int j = k0; j + m < nb; ++j) fresh += (j + m) < shared;
    if (available() < fresh) return plan;
    const std::vector<int> got = take(fresh);
    plan.ok = true;
    plan.table.assign(r.blocks.begin(), r.blocks.begin() + k0);
    int g = 0;
    for (int j = k0; j + m < nb; ++j) {
      const int src = r.blocks[j + m], dst = (j + m) < shared ? got[g++] : src;
      if (j == k0 && rem) {
        plan.moves.push_back({r.blocks[k0], dst, 0, rem, 0});
        plan.moves.push_back({src, dst, rem, bs, discard});
      } else {
        plan.moves.push_back({src, dst, 0, bs, discard});
      }
      plan.table.push_back(dst);
    }
    for (int j = k0; j < nb; ++j) {  // old blocks that the new table does not keep
      if (j < shared) shift_nodes_.push_back(r.nodes[j]);
      else if (j < k0 + m) shift_blocks_.push_back(r.blocks[j]);
    }
    if (shared > k0) r.nodes.resize(k0);
    r.blocks = plan.table;
    r.published = true;  // the blocks of a shifted cache are never published: only a prompt's prefill publishes
    return plan;
  }

  // The moves of every shift() since the last call are enqueued: release what they still read.
  void shift_done() {
    if (!shift_blocks_.empty()) alloc_.release(shift_blocks_);
    shift_blocks_.clear();
    if (!shift_nodes_.empty()) {
      ++clock_;
      for (auto it = shift_nodes_.rbegin(); it != shift_nodes_.rend(); ++it) {  // leaf first
        nodes_[*it].tick = clock_;
        unref_node(*it);
      }
    }
    shift_nodes_.clear();
  }

  // private blocks released by shift() and not yet returned by shift_done() (tests: they are in nobody's table)
  int shift_held_blocks() const { return (int)shift_blocks_.size(); }

  // ---------------------------------------------------------------------------------- prefix cache
  // Prompt tokens of a running request whose KV was found in the cache at its admission (shared blocks + fork).
  int cached_tokens(long long id) const { return reqs_.at(id).cached; }
  // Leading entries of the request's table that are index nodes (shared), the rest being private.
  int shared_blocks(long long id) const { return (int)reqs_.at(id).nodes.size(); }

  // The (src block, dst block) copies that the admissions since the last call ask for.  Their sources stay pinned
  // until copies_done(), which the engine calls once the copies are enqueued ahead of everything that follows.
  std::vector<std::pair<int, int>> take_copies() {
    std::vector<std::pair<int, int>> out;
    out.swap(copies_);
    return out;
  }
  void copies_done() {
    for (int n : pins_) unref_chain(n);
    pins_.clear();
    copies_.clear();
  }

  // Insert the request's full prompt blocks that the index does not hold yet as nodes held by the request (the
  // engine calls it once the prompt's last prefill chunk is launched).  A forked block is fully written by then
  // and is published like any other.  Where an equal node already exists the request keeps its duplicate, and
  // everything after it, private.  Returns the number of nodes inserted.
  int publish(long long id) {
    Req& r = reqs_.at(id);
    if (!r.cacheable || r.slot < 0 || r.published) return 0;
    r.published = true;
    const int bs = alloc_.block_size(), full = r.prompt_len / bs;
    ++clock_;
    int added = 0;
    for (int i = (int)r.nodes.size(); i < full; ++i) {
      const int parent = r.nodes.empty() ? 0 : r.nodes.back();
      if (find_child(parent, r.tokens.data() + (size_t)i * bs) >= 0) break;
      int n;
      if (!free_nodes_.empty()) {
        n = free_nodes_.back();
        free_nodes_.pop_back();
      } else {
        n = (int)nodes_.size();
        nodes_.emplace_back();
      }
      PrefixNode& nd = nodes_[n];
      nd.parent = parent;
      nd.toks.assign(r.tokens.begin() + (size_t)i * bs, r.tokens.begin() + (size_t)(i + 1) * bs);
      nd.block = r.blocks[i];
      nd.ref = 1;
      nd.children.clear();
      nd.tick = clock_;
      nd.live = true;
      nodes_[parent].children.push_back(n);
      r.nodes.push_back(n);
      ++num_cached_;
      ++added;
    }
    return added;
  }

  // Drop every unreferenced node (their blocks return to the free list).  Returns the number dropped.
  int reset_prefix_cache() {
    int n = 0;
    while (evict_one()) ++n;
    return n;
  }

  int cached_blocks() const { return num_cached_; }
  bool prefix_cache() const { return prefix_cache_; }
  int cow_min_tokens() const { return cow_min_; }

  // (block, references, children, last-use tick, parent's block or -1) of every cached node, by block id (tests).
  std::vector<std::vector<long long>> prefix_nodes() const {
    std::vector<std::vector<long long>> out;
    for (size_t n = 1; n < nodes_.size(); ++n) {
      const PrefixNode& nd = nodes_[n];
      if (nd.live)
        out.push_back({nd.block, nd.ref, (long long)nd.children.size(), nd.tick,
                       nd.parent > 0 ? nodes_[nd.parent].block : -1});
    }
    std::sort(out.begin(), out.end());
    return out;
  }

  std::vector<int> block_table(long long id) const { return reqs_.at(id).blocks; }
  int slot(long long id) const { return reqs_.at(id).slot; }
  std::vector<long long> slot_owners() const { return slots_; }
  std::vector<long long> running() const {
    std::vector<long long> out;
    for (long long s : slots_)
      if (s >= 0) out.push_back(s);
    return out;
  }
  int num_waiting() const { return (int)waiting_.size(); }
  int num_running() const {
    int n = 0;
    for (long long s : slots_) n += s >= 0;
    return n;
  }
  int highest_slot() const {
    for (int s = max_slots_ - 1; s >= 0; --s)
      if (slots_[s] >= 0) return s;
    return -1;
  }
  // blocks held by live requests (cached blocks that nobody references are allocatable, so they do not count)
  double kv_usage() const {
    return 1.0 - (double)available() / (double)(alloc_.num_blocks() - 1);
  }
  // allocatable blocks: the free list plus the cached blocks that nobody references (evicted on demand)
  int free_blocks() const { return available(); }
  int reserve_tokens() const { return reserve_tokens_; }

 private:
  struct Match {
    std::vector<int> chain;  // matched nodes, root's child first
    int src = -1;            // node to fork, or -1
    int p = 0;               // tokens the fork reuses
  };

  int available() const { return alloc_.num_free() + evictable_; }

  void ref_node(int n) {
    if (nodes_[n].ref++ == 0) --evictable_;
  }
  void unref_node(int n) {
    if (--nodes_[n].ref == 0) ++evictable_;
  }
  void ref_chain(int n) {
    for (; n > 0; n = nodes_[n].parent) ref_node(n);
  }
  void unref_chain(int n) {
    for (; n > 0; n = nodes_[n].parent) unref_node(n);
  }

  // child of `parent` whose token ids equal toks[0 .. block_size), or -1 (decided by the ids themselves)
  int find_child(int parent, const int* toks) const {
    for (int c : nodes_[parent].children)
      if (std::equal(nodes_[c].toks.begin(), nodes_[c].toks.end(), toks)) return c;
    return -1;
  }

  // Longest chain of cached blocks that prefixes the prompt, capped so that at least the last prompt token is
  // computed (and no more than the request's match_limit tokens are served), then the best partial match among the
  // last node's children (the fork), under the same cap.
  Match match(const Req& r) const {
    Match m;
    const int cap = r.match_limit < 0 ? r.prompt_len - 1 : std::min(r.match_limit, r.prompt_len - 1);
    const int bs = alloc_.block_size(), max_full = cap / bs;
    int node = 0;
    for (int i = 0; i < max_full; ++i) {
      const int c = find_child(node, r.tokens.data() + (size_t)i * bs);
      if (c < 0) break;
      m.chain.push_back(c);
      node = c;
    }
    const int base = (int)m.chain.size() * bs, limit = std::min(bs - 1, cap - base);
    for (int c : nodes_[node].children) {
      const std::vector<int>& t = nodes_[c].toks;
      int p = 0;
      while (p < limit && t[p] == r.tokens[base + p]) ++p;
      if (p > m.p) {
        m.p = p;
        m.src = c;
      }
    }
    if (m.p < cow_min_) {
      m.p = 0;
      m.src = -1;
    }
    return m;
  }

  // Evict the least recently used unreferenced leaf (ties: the lowest block id); false if there is none.
  bool evict_one() {
    int best = -1;
    for (int n = 1; n < (int)nodes_.size(); ++n) {
      const PrefixNode& nd = nodes_[n];
      if (!nd.live || nd.ref != 0 || !nd.children.empty()) continue;
      if (best < 0 || nd.tick < nodes_[best].tick || (nd.tick == nodes_[best].tick && nd.block < nodes_[best].block))
        best = n;
    }
    if (best < 0) return false;
    PrefixNode& nd = nodes_[best];
    std::vector<int>& sib = nodes_[nd.parent].children;
    sib.erase(std::find(sib.begin(), sib.end(), best));
    alloc_.release({nd.block});
    nd.live = false;
    nd.toks.clear();
    free_nodes_.push_back(best);
    --evictable_;
    --num_cached_;
    return true;
  }

  // n blocks from the free list, evicting cached blocks as needed (the caller checked available() >= n)
  std::vector<int> take(int n) {
    while (alloc_.num_free() < n)
      if (!evict_one()) throw std::runtime_error("KV cache exhausted");
    return alloc_.alloc(n);
  }

  // Return a request's private blocks to the free list and drop its references; unreferenced nodes stay cached.
  void release_blocks(Req& r) {
    const std::vector<int> priv(r.blocks.begin() + r.nodes.size(), r.blocks.end());
    if (!priv.empty()) alloc_.release(priv);
    if (!r.nodes.empty()) {
      ++clock_;
      for (int n : r.nodes) {
        nodes_[n].tick = clock_;
        unref_node(n);
      }
    }
    r.blocks.clear();
    r.nodes.clear();
    r.cached = 0;
    r.published = false;
  }

  BlockAllocator alloc_;
  int max_slots_, max_prefill_tokens_, max_blocks_per_seq_, reserve_tokens_;
  long long admit_counter_ = 0;
  std::vector<long long> slots_;
  std::deque<long long> waiting_;
  std::unordered_map<long long, Req> reqs_;
  // prefix cache
  bool prefix_cache_;
  int cow_min_;
  std::vector<PrefixNode> nodes_;  // [0] is the root
  std::vector<int> free_nodes_;
  int num_cached_ = 0, evictable_ = 0;
  long long clock_ = 0;
  std::vector<std::pair<int, int>> copies_;
  std::vector<int> pins_;
  // context shift: private blocks / index nodes released by shift(), held until shift_done()
  std::vector<int> shift_blocks_, shift_nodes_;
};
