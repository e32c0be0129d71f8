// block_cache.h -- the bookkeeping of the device cache of decoded blocks (include/longtail_hip.h, "a cache of decoded blocks"): which
// slot of the arena holds which block, who uses it, and which one goes next.  Host code without a line of HIP, beside restore_plan.h and
// restore_windows.h, so that a stand-alone program reaches it under a sanitizer (tests/san/block_cache_driver.cpp); restore.hip owns
// the arena and calls in here.
//
// A slot is FREE, RESERVED or VISIBLE.
//   VISIBLE   an ENTRY: the slot holds a block's chunks back to back, keyed by (hash identifier, block hash), with what a later session
//             compares before it trusts the bytes -- chunk count, raw size, a digest of the block's (chunk hash, chunk size) table -- and
//             whether the session that wrote it had verified the chunks.  Only entries are found by lookup().
//   RESERVED  a session is writing the slot; nobody finds it.  commit() makes it an entry, abort() frees it.
//   pins      sessions that read an entry.  A pinned entry and a reserved slot are never taken.
// reserve() takes, in this order: the slot of the entry with the same key when it is not pinned (the caller found it not to match, or
// did not look: its bytes are about to be replaced), none when that entry is pinned, the free slot with the lowest index, the entry
// that is not pinned and was used longest ago.  "Used" is pin() or commit(), numbered by one counter: the order is strict and a model
// predicts it exactly (tests/block_cache_util.py).
// commit() of a key that has an entry in ANOTHER slot (two sessions reserved the same block): the older entry goes when it is not
// pinned, otherwise the new slot is freed and the older entry stays.  There is one entry per key at any time.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

namespace block_cache
{

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

struct Key
{
    uint32_t hash_identifier;
    uint64_t block_hash;
    bool operator==(const Key& o) const { return hash_identifier == o.hash_identifier && block_hash == o.block_hash; }
};
struct KeyHasher
{
    size_t operator()(const Key& k) const { return (size_t)((k.block_hash ^ ((uint64_t)k.hash_identifier << 32)) * 0x9E3779B97F4A7C15ull >> 16); }
};
struct Meta
{
    uint32_t chunks, raw;
    uint64_t digest;
    bool operator==(const Meta& o) const { return chunks == o.chunks && raw == o.raw && digest == o.digest; }
};

// FNV-1a over the block's chunk table as the StoreIndex lists it: per chunk its hash (8 bytes, little end first) and its size (4 bytes)
inline uint64_t table_digest(const uint64_t* chunk_hashes, const uint32_t* chunk_sizes, uint32_t chunks)
{
    uint64_t h = 0xCBF29CE484222325ull;
    const auto mix = [&h](uint64_t v, int bytes) {
        for (int i = 0; i < bytes; ++i)
            h = (h ^ ((v >> (8 * i)) & 0xFFu)) * 0x100000001B3ull;
    };
    for (uint32_t j = 0; j < chunks; ++j)
        mix(chunk_hashes[j], 8), mix(chunk_sizes[j], 4);
    return h;
}

enum State : uint8_t
{
    FREE = 0,
    RESERVED = 1,
    VISIBLE = 2
};
struct Slot
{
    State state = FREE;
    bool verified = false;
    uint32_t pins = 0;
    Key key = {0, 0};
    Meta meta = {0, 0, 0};
    uint64_t used = 0;
};
struct Counts
{
    uint64_t hits = 0, inserted = 0, evicted = 0, bypassed = 0, dropped = 0;
};

class Table
{
  public:
    // (a slot's size is rounded up to a multiple of 64)
    Table(uint32_t slot_count, uint64_t slot_bytes) : slots_(slot_count), slot_bytes_((slot_bytes + 63u) & ~(uint64_t)63u) {}

    uint32_t slot_count() const { return (uint32_t)slots_.size(); }
    uint64_t slot_bytes() const { return slot_bytes_; }
    const Slot& slot(uint32_t s) const { return slots_[s]; }
    const Counts& counts() const { return counts_; }
    uint64_t resident() const { return index_.size(); }
    uint64_t pinned() const
    {
        return (uint64_t)std::count_if(slots_.begin(), slots_.end(), [](const Slot& s) { return s.state == VISIBLE && s.pins; });
    }
    uint64_t reserved() const
    {
        return (uint64_t)std::count_if(slots_.begin(), slots_.end(), [](const Slot& s) { return s.state == RESERVED; });
    }

    // the entry of `key`, or NO_SLOT
    uint32_t lookup(const Key& key) const
    {
        const auto it = index_.find(key);
        return it == index_.end() ? NO_SLOT : it->second;
    }
    // may a session that expects `meta` read entry s?  A verifying session reads only what a verifying session wrote.
    bool matches(uint32_t s, const Meta& meta, bool need_verified) const
    {
        return s < slots_.size() && slots_[s].state == VISIBLE && slots_[s].meta == meta && (!need_verified || slots_[s].verified);
    }
    bool pin(uint32_t s)
    {
        if (s >= slots_.size() || slots_[s].state != VISIBLE)
            return false;
        ++slots_[s].pins;
        slots_[s].used = ++clock_;
        ++counts_.hits;
        return true;
    }
    bool unpin(uint32_t s)
    {
        if (s >= slots_.size() || slots_[s].state != VISIBLE || !slots_[s].pins)
            return false;
        --slots_[s].pins;
        return true;
    }
    // a slot for the block to be written into, or NO_SLOT: the block is bypassed (too large, its entry is pinned, nothing can be taken)
    uint32_t reserve(const Key& key, const Meta& meta)
    {
        uint32_t s = NO_SLOT;
        if ((uint64_t)meta.raw <= slot_bytes_)
        {
            const uint32_t mine = lookup(key);
            if (mine != NO_SLOT)
                s = slots_[mine].pins ? NO_SLOT : mine;
            else
            {
                for (uint32_t i = 0; i < slots_.size() && s == NO_SLOT; ++i)
                    if (slots_[i].state == FREE)
                        s = i;
                if (s == NO_SLOT)
                    for (uint32_t i = 0; i < slots_.size(); ++i)
                        if (slots_[i].state == VISIBLE && !slots_[i].pins && (s == NO_SLOT || slots_[i].used < slots_[s].used))
                            s = i;
            }
        }
        if (s == NO_SLOT)
        {
            ++counts_.bypassed;
            return NO_SLOT;
        }
        if (slots_[s].state == VISIBLE)
            evict(s);
        slots_[s].state = RESERVED;
        slots_[s].key = key;
        slots_[s].meta = meta;
        return s;
    }
    // a reserved slot becomes the entry of its key; false: another slot's pinned entry of that key stays, and this slot is freed
    bool commit(uint32_t s, bool verified)
    {
        if (s >= slots_.size() || slots_[s].state != RESERVED)
            return false;
        const uint32_t other = lookup(slots_[s].key);
        if (other != NO_SLOT)
        {
            if (slots_[other].pins)
            {
                slots_[s] = Slot();
                ++counts_.bypassed;
                return false;
            }
            evict(other);
        }
        slots_[s].state = VISIBLE;
        slots_[s].verified = verified;
        slots_[s].pins = 0;
        slots_[s].used = ++clock_;
        index_[slots_[s].key] = s;
        ++counts_.inserted;
        return true;
    }
    // a reserved slot is given back; bad: the block it was reserved for was found bad
    bool abort(uint32_t s, bool bad)
    {
        if (s >= slots_.size() || slots_[s].state != RESERVED)
            return false;
        slots_[s] = Slot();
        if (bad)
            ++counts_.dropped;
        return true;
    }
    // every entry goes; false (and nothing changes) while an entry is pinned or a slot is reserved
    bool clear()
    {
        if (pinned() || reserved())
            return false;
        for (Slot& s : slots_)
            s = Slot();
        index_.clear();
        return true;
    }
    // the entries' slots, least recently used first
    std::vector<uint32_t> lru_order() const
    {
        std::vector<uint32_t> order;
        for (uint32_t i = 0; i < slots_.size(); ++i)
            if (slots_[i].state == VISIBLE)
                order.push_back(i);
        std::sort(order.begin(), order.end(), [this](uint32_t a, uint32_t b) { return slots_[a].used < slots_[b].used; });
        return order;
    }

  private:
    void evict(uint32_t s)
    {
        index_.erase(slots_[s].key);
        slots_[s] = Slot();
        ++counts_.evicted;
    }
    std::vector<Slot> slots_;
    uint64_t slot_bytes_;
    std::unordered_map<Key, uint32_t, KeyHasher> index_;
    uint64_t clock_ = 0;
    Counts counts_;
};

} // namespace block_cache
