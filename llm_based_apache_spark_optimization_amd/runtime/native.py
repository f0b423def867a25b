"""Loader for the native host runtime (``_lsa_runtime``: scheduler, KV allocator, edit distance).

The extension is built in-tree by ``ops.build.build_runtime`` (g++, a few seconds).  A fresh checkout
builds it on first import; only if no C++ toolchain is present does it fall back to the equivalent
pure-Python classes below (identical semantics, used by nothing on the hot path).
"""
from __future__ import annotations

import collections
import importlib
import logging

log = logging.getLogger(__name__)


def _load():
    try:
        return importlib.import_module(__package__ + "._lsa_runtime")
    except ImportError:
        pass
    try:
        from ..ops.build import build_runtime

        build_runtime()
        return importlib.import_module(__package__ + "._lsa_runtime")
    except Exception as e:  # noqa: BLE001
        log.warning("native runtime unavailable (%s); using the Python fallback", e)
        return None


_mod = _load()
NATIVE = _mod is not None


class _PyBlockAllocator:
    def __init__(self, num_blocks: int, block_size: int = 64):
        if num_blocks < 2:
            raise ValueError("need at least 2 KV blocks (block 0 is scratch)")
        self.num_blocks, self.block_size = num_blocks, block_size
        self._free = list(range(num_blocks - 1, 0, -1))
        self._owned = set()

    def blocks_for(self, tokens):
        return (tokens + self.block_size - 1) // self.block_size

    def can_alloc(self, n):
        return len(self._free) >= n

    def alloc(self, n):
        if n < 0:
            raise ValueError("negative block count")
        if not self.can_alloc(n):
            raise RuntimeError("KV cache exhausted")
        if n == 0:
            return []
        out = self._free[-n:][::-1]
        del self._free[-n:]
        self._owned.update(out)
        return out

    def release(self, blocks):
        blocks = list(blocks)
        if any(b <= 0 or b >= self.num_blocks or b not in self._owned for b in blocks):
            raise ValueError("bad or already-free block id")
        if len(set(blocks)) != len(blocks):
            raise ValueError("block listed twice")
        for b in blocks:
            self._owned.discard(b)
            self._free.append(b)

    @property
    def num_free(self):
        return len(self._free)


class _PyScheduler:
    """Pure-Python twin of csrc/runtime/runtime_core.h Scheduler (lazy KV reservation + preemption + the prefix
    cache: see the comment there for the index, its safety invariant and the eviction rule)."""

    COW_MIN_TOKENS = 8  # Scheduler::kCowMinTokens (the measurement behind it is quoted there)

    def __init__(self, num_blocks, block_size, max_slots, max_prefill_tokens, max_blocks_per_seq, reserve_tokens=64,
                 prefix_cache=False, cow_min_tokens=COW_MIN_TOKENS):
        self._alloc = _PyBlockAllocator(num_blocks, block_size)
        self._max_slots, self._budget, self._maxb = max_slots, max_prefill_tokens, max_blocks_per_seq
        self._reserve = reserve_tokens
        self._slots = [-1] * max_slots
        self._waiting = collections.deque()
        self._reqs = {}
        self._admits = 0
        # prefix cache: node id -> {parent, toks, block, ref, children (insertion order), tick}; 0 is the root
        self._cache, self._cow_min = bool(prefix_cache), max(1, int(cow_min_tokens))
        self._nodes = {0: {"parent": -1, "toks": (), "block": -1, "ref": 0, "children": [], "tick": 0}}
        self._next_node = 1
        self._evictable = 0
        self._clock = 0
        self._copies, self._pins = [], []
        self._shift_blocks, self._shift_nodes = [], []  # released by shift(), held until shift_done()

    def add(self, rid, prompt_len, max_new, tokens=(), cacheable=True, match_limit=-1):
        if rid in self._reqs:
            raise ValueError("duplicate request id")
        if prompt_len < 1 or max_new < 1:
            raise ValueError("empty prompt or max_new < 1")
        need = self._alloc.blocks_for(prompt_len + max_new)
        if need > self._maxb:
            raise ValueError("request exceeds max model length")
        if need > self._alloc.num_blocks - 1:
            raise ValueError("request larger than the whole KV cache")
        cache = self._cache and cacheable
        if cache and len(tokens) != prompt_len:
            raise ValueError("tokens must hold prompt_len ids")
        self._reqs[rid] = {"p": prompt_len, "n": max_new, "slot": -1, "blocks": [], "seq": -1,
                           "tokens": [int(t) for t in tokens] if cache else [], "cacheable": cache,
                           "published": False, "cached": 0, "nodes": [],
                           "match_limit": int(match_limit) if cache else -1}
        self._waiting.append(rid)

    def _admit_blocks(self, r):
        gen = r["n"] if self._reserve < 0 else min(r["n"], self._reserve)
        return self._alloc.blocks_for(r["p"] + gen)

    # ------------------------------------------------------------------------------ prefix cache
    def _available(self):
        return self._alloc.num_free + self._evictable

    def _ref(self, n):
        nd = self._nodes[n]
        if nd["ref"] == 0:
            self._evictable -= 1
        nd["ref"] += 1

    def _unref(self, n):
        nd = self._nodes[n]
        nd["ref"] -= 1
        if nd["ref"] == 0:
            self._evictable += 1

    def _chain_of(self, n):
        while n > 0:
            yield n
            n = self._nodes[n]["parent"]

    def _find_child(self, parent, toks):
        for c in self._nodes[parent]["children"]:
            if self._nodes[c]["toks"] == toks:
                return c
        return -1

    def _match(self, r):
        """(chain, src, p): the longest chain of cached blocks that prefixes the prompt (at least the last prompt
        token stays to be computed, and no more than the request's ``match_limit`` tokens are served), then the best
        partial match among the last node's children (the fork), under the same cap."""
        bs, toks = self._alloc.block_size, r["tokens"]
        cap = r["p"] - 1 if r["match_limit"] < 0 else min(r["match_limit"], r["p"] - 1)
        chain, node = [], 0
        for i in range(cap // bs):
            c = self._find_child(node, tuple(toks[i * bs:(i + 1) * bs]))
            if c < 0:
                break
            chain.append(c)
            node = c
        base = len(chain) * bs
        limit = min(bs - 1, cap - base)
        best, src = 0, -1
        for c in self._nodes[node]["children"]:
            t, p = self._nodes[c]["toks"], 0
            while p < limit and t[p] == toks[base + p]:
                p += 1
            if p > best:
                best, src = p, c
        if best < self._cow_min:
            best, src = 0, -1
        return chain, src, best

    def _evict_one(self):
        best = -1
        for n, nd in self._nodes.items():
            if n == 0 or nd["ref"] != 0 or nd["children"]:
                continue
            if best < 0 or (nd["tick"], nd["block"]) < (self._nodes[best]["tick"], self._nodes[best]["block"]):
                best = n
        if best < 0:
            return False
        nd = self._nodes.pop(best)
        self._nodes[nd["parent"]]["children"].remove(best)
        self._alloc.release([nd["block"]])
        self._evictable -= 1
        return True

    def _take(self, n):
        while self._alloc.num_free < n:
            if not self._evict_one():
                raise RuntimeError("KV cache exhausted")
        return self._alloc.alloc(n)

    def _release_blocks(self, r):
        priv = r["blocks"][len(r["nodes"]):]
        if priv:
            self._alloc.release(priv)
        if r["nodes"]:
            self._clock += 1
            for n in r["nodes"]:
                self._nodes[n]["tick"] = self._clock
                self._unref(n)
        r.update(blocks=[], nodes=[], cached=0, published=False)

    def cached_tokens(self, rid):
        return self._reqs[rid]["cached"]

    def shared_blocks(self, rid):
        return len(self._reqs[rid]["nodes"])

    def take_copies(self):
        out, self._copies = self._copies, []
        return out

    def copies_done(self):
        for n in self._pins:
            for a in list(self._chain_of(n)):
                self._unref(a)
        self._pins, self._copies = [], []

    def publish(self, rid):
        r = self._reqs[rid]
        if not r["cacheable"] or r["slot"] < 0 or r["published"]:
            return 0
        r["published"] = True
        bs = self._alloc.block_size
        self._clock += 1
        added = 0
        for i in range(len(r["nodes"]), r["p"] // bs):
            parent = r["nodes"][-1] if r["nodes"] else 0
            toks = tuple(r["tokens"][i * bs:(i + 1) * bs])
            if self._find_child(parent, toks) >= 0:
                break
            n, self._next_node = self._next_node, self._next_node + 1
            self._nodes[n] = {"parent": parent, "toks": toks, "block": r["blocks"][i], "ref": 1, "children": [],
                              "tick": self._clock}
            self._nodes[parent]["children"].append(n)
            r["nodes"].append(n)
            added += 1
        return added

    def reset_prefix_cache(self):
        n = 0
        while self._evict_one():
            n += 1
        return n

    @property
    def cached_blocks(self):
        return len(self._nodes) - 1

    @property
    def prefix_cache(self):
        return self._cache

    @property
    def cow_min_tokens(self):
        return self._cow_min

    def prefix_nodes(self):
        return sorted([nd["block"], nd["ref"], len(nd["children"]), nd["tick"],
                       self._nodes[nd["parent"]]["block"] if nd["parent"] > 0 else -1]
                      for n, nd in self._nodes.items() if n)

    # ------------------------------------------------------------------------------ scheduling
    def admit(self):
        out, budget = [], self._budget
        bs = self._alloc.block_size
        while self._waiting:
            r = self._reqs[self._waiting[0]]
            chain, src, p = self._match(r) if r["cacheable"] else ([], -1, 0)
            cached = len(chain) * bs + p
            if out and r["p"] - cached > budget:
                break
            need = self._admit_blocks(r) - len(chain)
            pinned = chain + (list(self._chain_of(src)) if src >= 0 else [])
            for n in pinned:
                self._ref(n)
            try:
                slot = self._slots.index(-1)
            except ValueError:
                slot = -1
            if self._available() < need or slot < 0:
                for n in pinned:
                    self._unref(n)
                break
            rid = self._waiting.popleft()
            if r["cacheable"]:
                self._clock += 1
            for n in chain:
                self._nodes[n]["tick"] = self._clock
            priv = self._take(need)
            if src >= 0:
                self._nodes[src]["tick"] = self._clock
                self._copies.append((self._nodes[src]["block"], priv[0]))
                self._pins.append(src)
            self._admits += 1
            r.update(nodes=list(chain), blocks=[self._nodes[n]["block"] for n in chain] + priv, cached=cached,
                     slot=slot, seq=self._admits)
            self._slots[slot] = rid
            budget -= r["p"] - cached
            out.append(rid)
        return out

    def grow(self, rid, tokens):
        r = self._reqs[rid]
        if r["slot"] < 0:
            raise ValueError("grow: request is not running")
        want = min(self._alloc.blocks_for(min(tokens, r["p"] + r["n"])), self._maxb)
        add = want - len(r["blocks"])
        if add <= 0:
            return 0
        if self._available() < add:
            return -1
        r["blocks"] += self._take(add)
        return add

    def shift(self, rid, keep, discard):
        """Scheduler::shift: (moves, new table) of a context shift, or None when the fresh blocks it needs cannot be
        supplied (nothing changes then).  The blocks it releases are held until ``shift_done``."""
        r = self._reqs[rid]
        bs, nb = self._alloc.block_size, len(r["blocks"])
        if r["slot"] < 0:
            raise ValueError("shift: request is not running")
        if keep < 0 or discard <= 0 or discard % bs:
            raise ValueError("shift: bad keep or discard")
        k0, rem, m, shared = keep // bs, keep % bs, discard // bs, len(r["nodes"])
        if k0 + m >= nb:
            raise ValueError("shift: nothing left behind the discarded tokens")
        fresh = sum(1 for j in range(k0, nb - m) if j + m < shared)
        if self._available() < fresh:
            return None
        got = self._take(fresh)
        moves, table, g = [], r["blocks"][:k0], 0
        for j in range(k0, nb - m):
            src = dst = r["blocks"][j + m]
            if j + m < shared:
                dst, g = got[g], g + 1
            if j == k0 and rem:
                moves.append((r["blocks"][k0], dst, 0, rem, 0))
                moves.append((src, dst, rem, bs, discard))
            else:
                moves.append((src, dst, 0, bs, discard))
            table.append(dst)
        for j in range(k0, nb):
            if j < shared:
                self._shift_nodes.append(r["nodes"][j])
            elif j < k0 + m:
                self._shift_blocks.append(r["blocks"][j])
        del r["nodes"][k0:]
        r["blocks"] = table
        r["published"] = True  # the blocks of a shifted cache are never published
        return moves, list(table)

    def shift_done(self):
        if self._shift_blocks:
            self._alloc.release(self._shift_blocks)
        if self._shift_nodes:
            self._clock += 1
            for n in reversed(self._shift_nodes):
                self._nodes[n]["tick"] = self._clock
                self._unref(n)
        self._shift_blocks, self._shift_nodes = [], []

    def preempt(self, rid, prompt_len, max_new, tokens=(), match_limit=-1):
        r = self._reqs[rid]
        if r["slot"] < 0:
            raise ValueError("preempt: request is not running")
        if prompt_len < 1 or max_new < 1 or self._alloc.blocks_for(prompt_len + max_new) > self._maxb:
            raise ValueError("preempt: bad resumed lengths")
        if r["cacheable"] and len(tokens) != prompt_len:
            raise ValueError("tokens must hold prompt_len ids")
        self._slots[r["slot"]] = -1
        self._release_blocks(r)
        r.update(slot=-1, seq=-1, p=prompt_len, n=max_new, match_limit=int(match_limit))
        if r["cacheable"]:
            r["tokens"] = [int(t) for t in tokens]
        self._waiting.appendleft(rid)

    def youngest_first(self):
        return sorted((s for s in self._slots if s >= 0), key=lambda rid: -self._reqs[rid]["seq"])

    def finish(self, rid):
        r = self._reqs.pop(rid, None)
        if r is None:
            return
        if r["slot"] >= 0:
            self._slots[r["slot"]] = -1
        self._release_blocks(r)
        if rid in self._waiting:
            self._waiting.remove(rid)

    def block_table(self, rid):
        return list(self._reqs[rid]["blocks"])

    def slot(self, rid):
        return self._reqs[rid]["slot"]

    def slot_owners(self):
        return list(self._slots)

    def running(self):
        return [s for s in self._slots if s >= 0]

    @property
    def num_waiting(self):
        return len(self._waiting)

    @property
    def num_running(self):
        return sum(1 for s in self._slots if s >= 0)

    @property
    def highest_slot(self):
        for i in range(self._max_slots - 1, -1, -1):
            if self._slots[i] >= 0:
                return i
        return -1

    @property
    def kv_usage(self):
        return 1.0 - self._available() / (self._alloc.num_blocks - 1)

    @property
    def free_blocks(self):
        return self._available()

    @property
    def reserve_tokens(self):
        return self._reserve


def _py_levenshtein(a: str, b: str) -> int:
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


if NATIVE:
    Scheduler = _mod.Scheduler
    BlockAllocator = _mod.BlockAllocator
    levenshtein = _mod.levenshtein
    levenshtein_batch = _mod.levenshtein_batch
else:  # pragma: no cover - only without a C++ toolchain
    Scheduler = _PyScheduler
    BlockAllocator = _PyBlockAllocator
    levenshtein = _py_levenshtein

    def levenshtein_batch(a, b):
        return [_py_levenshtein(x, y) for x, y in zip(a, b)]
