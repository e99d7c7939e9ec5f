// The open-addressing table of 63-bit keys that csrc/voxel.hip (voxel-grid downsampling) and csrc/sparse_conv.hip (stride and kernel maps) share:
// 64-bit words, capacity a power of two, linear probing from a mixed hash, the all-ones word marks an empty slot (no 63-bit key is all ones).
// Every probe loop is bounded by the capacity: no input spins a wave forever; -1 = the table is full (insert) or the key is absent (find).
// Included inside a translation unit's anonymous namespace.
#pragma once

constexpr unsigned long long EMPTY = ~0ull;

// murmur3's 64-bit finaliser: keys that differ in one axis' top bits only, or run along a line, spread over the table
__device__ __forceinline__ unsigned long long mix64(unsigned long long h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// the slot that holds `key` after the call (claimed by a 64-bit compare-and-swap, or found), or -1 if every slot holds another key
__device__ __forceinline__ long long hash_insert(unsigned long long *__restrict__ keys, size_t cap, unsigned long long key) {
    size_t s = (size_t)mix64(key) & (cap - 1);
    for (size_t probe = 0; probe < cap; ++probe) {
        const unsigned long long prev = atomicCAS(&keys[s], EMPTY, key);
        if (prev == EMPTY || prev == key) return (long long)s;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

// the slot that holds `key` in a table no lane is inserting into, or -1
__device__ __forceinline__ long long hash_find(const unsigned long long *__restrict__ keys, size_t cap, unsigned long long key) {
    size_t s = (size_t)mix64(key) & (cap - 1);
    for (size_t probe = 0; probe < cap; ++probe) {
        const unsigned long long have = keys[s];
        if (have == key) return (long long)s;
        if (have == EMPTY) return -1;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}
