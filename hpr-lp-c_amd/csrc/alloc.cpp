// alloc.cpp -- process-wide cache of large freed device blocks (common.h: why), and the arena of a group of solvers created
// together (common.h: Arena).
//
// A block belongs to the device it was allocated on, whatever device the freeing thread has current: put() asks the
// runtime for the owner (hipPointerGetAttributes), waits for THAT device and files the block under it; get() serves the
// calling thread's current device, like hipMalloc.  The cap is per device and bounded by a third of the device's memory.
#include <map>
#include <mutex>

#include <memory>

#include "common.h"
#include "env.h"
#include "hprlp_amd.h"

namespace hprlp {

namespace {

// The bookkeeping, free of HIP calls (hprlp_alloc_cache_selftest exercises it without a GPU).
struct BlockIndex {
    std::multimap<std::pair<int, size_t>, void *> blocks;  // (owning device, capacity) -> block
    std::map<int, size_t> bytes;                           // per device
    // smallest cached block of `dev` that holds the request and wastes at most a quarter of itself
    void *take(int dev, size_t want, size_t *capacity) {
        auto it = blocks.lower_bound({dev, want});
        if (it == blocks.end() || it->first.first != dev || it->first.second > want + want / 3) return nullptr;
        void *p = it->second;
        *capacity = it->first.second;
        bytes[dev] -= it->first.second;
        blocks.erase(it);
        return p;
    }
    bool file(int dev, size_t capacity, void *p, size_t cap_per_device) {
        if (bytes[dev] + capacity > cap_per_device) return false;
        blocks.insert({{dev, capacity}, p});
        bytes[dev] += capacity;
        return true;
    }
    size_t held(int dev) const {
        auto it = bytes.find(dev);
        return it == bytes.end() ? 0 : it->second;
    }
};

struct Cache {
    std::mutex mu;
    BlockIndex idx;
    std::map<int, size_t> cap;  // per device: min(kDeviceCacheCapBytes, total memory / 3)
    bool off = false;
    Cache() {
        const char *e = env_get("HPRLP_NO_ALLOC_CACHE");
        off = e && e[0] == '1';
    }
};

Cache &cache() {
    static Cache c;
    return c;
}

// RAII: make `dev` current, restore the caller's device on exit
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (switched) (void)hipSetDevice(prev);
    }
};

}  // namespace

void *device_cache_get(size_t bytes, size_t *capacity) {
    Cache &c = cache();
    if (c.off) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(c.mu);
    return c.idx.take(dev, bytes, capacity);
}

bool device_cache_put(void *p, size_t capacity) {
    Cache &c = cache();
    if (c.off || !p) return false;
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const int owner = attr.device;
    DeviceScope scope(owner);
    // hipFree waits for the device; code that frees a buffer right behind the kernels that used it relies on that
    if (hipDeviceSynchronize() != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.cap.find(owner);
    if (it == c.cap.end()) {
        size_t free_b = 0, total_b = 0;
        size_t cap = kDeviceCacheCapBytes;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) cap = std::min(cap, total_b / 3);
        it = c.cap.emplace(owner, cap).first;
    }
    return c.idx.file(owner, capacity, p, it->second);
}

void device_cache_trim() {
    Cache &c = cache();
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto &kv : c.idx.blocks) {
        DeviceScope scope(kv.first.first);
        (void)hipFree(kv.second);
    }
    c.idx.blocks.clear();
    c.idx.bytes.clear();
}

void *device_malloc_or_trim(size_t bytes) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
        // the cache may be sitting on the memory this request needs (blocks of other size classes): give it back, retry once
        (void)hipGetLastError();
        device_cache_trim();
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " in hipMalloc of " + std::to_string(bytes) + " bytes");
    return p;
}

// ---- arena ------------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kArenaAlign = 256;
constexpr size_t kArenaBlockBytes = size_t(16) << 20;   // device blocks (and their mirrors)
constexpr size_t kArenaPinnedBytes = size_t(256) << 10;  // pinned blocks of the members' scalar blocks

// The bookkeeping of one bump allocator over a list of blocks, free of HIP calls (hprlp_arena_selftest exercises it without a
// GPU): where a request lands, when a further block is needed and how large it has to be.
struct BumpIndex {
    size_t block_bytes;
    std::vector<size_t> cap, used;  // per block
    long refs = 1;                  // the creator's; one more per solver created in the arena
    explicit BumpIndex(size_t block_bytes_) : block_bytes(block_bytes_) {}
    static size_t aligned(size_t bytes) { return (std::max<size_t>(bytes, 1) + kArenaAlign - 1) / kArenaAlign * kArenaAlign; }
    // capacity of the block a request needs when the last one is full: the ordinary size, or the request's own if it is larger
    size_t next_block_bytes(size_t bytes) const { return std::max(block_bytes, aligned(bytes)); }
    bool fits_last(size_t bytes) const { return !cap.empty() && used.back() + aligned(bytes) <= cap.back(); }
    void add_block(size_t capacity) {
        cap.push_back(capacity);
        used.push_back(0);
    }
    // {block, offset} of the request inside the last block (the caller has made sure it fits)
    std::pair<size_t, size_t> take(size_t bytes) {
        const size_t off = used.back();
        used.back() += aligned(bytes);
        return {cap.size() - 1, off};
    }
    void retain() { ++refs; }
    bool release() { return --refs == 0; }  // true: the last user is gone
};

thread_local Arena *g_arena_scope = nullptr;

}  // namespace

struct Arena {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;  // (members may be destroyed from any thread)
    BumpIndex dev{kArenaBlockBytes}, pin{kArenaPinnedBytes};
    std::vector<char *> dev_blocks, mirrors, pin_blocks;  // mirrors[b]: pinned copy of dev_blocks[b] until flush(), then null
};

AllocCounts &alloc_counts() {
    thread_local AllocCounts c;
    return c;
}

Arena *arena_create(int device) {
    std::unique_ptr<Arena> a(new Arena());
    a->device = device;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreate(&a->stream));
    return a.release();
}

void arena_retain(Arena *a) {
    std::lock_guard<std::mutex> lock(a->mu);
    a->dev.retain();
}

void arena_release(Arena *a) {
    if (!a) return;
    {
        std::lock_guard<std::mutex> lock(a->mu);
        if (!a->dev.release()) return;
    }
    DeviceScope scope(a->device);
    for (char *m : a->mirrors)
        if (m) (void)hipHostFree(m);
    for (char *b : a->dev_blocks) {
        const auto t0 = time_now();
        (void)hipFree(b);  // (waits for the device: nothing of a member is in flight afterwards)
        AllocStats::get().free_s += time_since(t0);
        ++AllocStats::get().frees;
        ++alloc_counts().device_frees;
    }
    for (char *b : a->pin_blocks) (void)hipHostFree(b);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

hipStream_t arena_stream(Arena *a) { return a->stream; }

ArenaScope::ArenaScope(Arena *a) : prev(g_arena_scope) { g_arena_scope = a; }
ArenaScope::~ArenaScope() { g_arena_scope = prev; }
Arena *arena_in_scope() { return g_arena_scope; }

void *arena_alloc(Arena *a, size_t bytes) {
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->dev.fits_last(bytes)) {
        const size_t cap = a->dev.next_block_bytes(bytes);
        const auto t0 = time_now();
        char *d = static_cast<char *>(device_malloc_or_trim(cap));
        AllocStats::get().malloc_s += time_since(t0);
        ++AllocStats::get().mallocs;
        ++alloc_counts().device_allocs;
        char *h = nullptr;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&h), cap, hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipFree(d);
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " in hipHostMalloc of an arena mirror");
        }
        ++alloc_counts().pinned_allocs;
        std::memset(h, 0, cap);
        a->dev.add_block(cap);
        a->dev_blocks.push_back(d);
        a->mirrors.push_back(h);
    }
    const std::pair<size_t, size_t> at = a->dev.take(bytes);
    return a->dev_blocks[at.first] + at.second;
}

void *arena_alloc_pinned(Arena *a, size_t bytes) {
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->pin.fits_last(bytes)) {
        const size_t cap = a->pin.next_block_bytes(bytes);
        char *h = nullptr;
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h), cap, hipHostMallocDefault));
        ++alloc_counts().pinned_allocs;
        std::memset(h, 0, cap);
        a->pin.add_block(cap);
        a->pin_blocks.push_back(h);
    }
    const std::pair<size_t, size_t> at = a->pin.take(bytes);
    return a->pin_blocks[at.first] + at.second;
}

// the mirror address of a device address inside a block still to be sent, or null
static char *mirror_of(Arena *a, const void *p, size_t bytes) {
    const char *q = static_cast<const char *>(p);
    for (size_t b = 0; b < a->dev_blocks.size(); ++b)
        if (a->mirrors[b] && q >= a->dev_blocks[b] && q + bytes <= a->dev_blocks[b] + a->dev.used[b]) return a->mirrors[b] + (q - a->dev_blocks[b]);
    return nullptr;
}

bool arena_upload(Arena *a, void *dst, const void *src, size_t bytes) {
    if (!a) return false;
    std::lock_guard<std::mutex> lock(a->mu);
    char *m = mirror_of(a, dst, bytes);
    if (!m) return false;
    std::memcpy(m, src, bytes);
    return true;
}

bool arena_mirrored(Arena *a, const void *p) {
    if (!a) return false;
    std::lock_guard<std::mutex> lock(a->mu);
    return mirror_of(a, p, 1) != nullptr;
}

void arena_flush(Arena *a) {
    std::lock_guard<std::mutex> lock(a->mu);
    DeviceScope scope(a->device);
    bool sent = false;
    for (size_t b = 0; b < a->dev_blocks.size(); ++b) {
        if (!a->mirrors[b] || a->dev.used[b] == 0) continue;
        HIP_CHECK(hipMemcpyAsync(a->dev_blocks[b], a->mirrors[b], a->dev.used[b], hipMemcpyHostToDevice, a->stream));
        ++alloc_counts().h2d_copies;
        sent = true;
    }
    if (sent) HIP_CHECK(hipStreamSynchronize(a->stream));
    for (char *&m : a->mirrors) {
        if (m) (void)hipHostFree(m);
        m = nullptr;
    }
}

}  // namespace hprlp

extern "C" void hprlp_release_device_cache(void) { hprlp::device_cache_trim(); }

// Bookkeeping self-test of the arena without a GPU (tests/test_many_setup_cpu.py): alignment, growth by a further block, a request
// larger than a block, the reference count.  Returns 0 on success, the number of the failed check otherwise.
extern "C" int hprlp_arena_selftest(void) {
    using hprlp::BumpIndex;
    const size_t KiB = 1024;
    BumpIndex ix(64 * KiB);
    if (ix.fits_last(1)) return 1;                                   // no block yet
    if (ix.next_block_bytes(100) != 64 * KiB) return 2;
    ix.add_block(ix.next_block_bytes(100));
    const auto a = ix.take(100), b = ix.take(1), c = ix.take(256), d = ix.take(0);
    if (a.first != 0 || a.second != 0) return 3;
    if (b.second != 256 || c.second != 512 || d.second != 768) return 4;  // every piece starts on a 256-byte boundary; an empty one takes a slot
    if (ix.used[0] != 1024) return 5;
    if (!ix.fits_last(63 * KiB) || ix.fits_last(63 * KiB + 1)) return 6;   // to the last byte of the block, not past it
    const size_t want = 63 * KiB + 1;
    ix.add_block(ix.next_block_bytes(want));                          // growth by a further block
    const auto e = ix.take(want);
    if (e.first != 1 || e.second != 0 || ix.cap[1] != 64 * KiB || ix.used[1] != 63 * KiB + 256) return 7;
    if (ix.used[0] != 1024) return 8;                                 // (the earlier block keeps what it handed out)
    if (!ix.fits_last(768) || ix.fits_last(769)) return 9;
    if (ix.next_block_bytes(200 * KiB + 1) != 200 * KiB + 256) return 10;  // a request larger than a block gets a block of its own size
    ix.add_block(ix.next_block_bytes(200 * KiB + 1));
    const auto f = ix.take(200 * KiB + 1);
    if (f.first != 2 || f.second != 0 || !(ix.used[2] <= ix.cap[2])) return 11;
    // the reference count: the creator's, three members; the blocks go when the last of them has gone, in any order
    ix.retain(); ix.retain(); ix.retain();
    if (ix.refs != 4) return 12;
    if (ix.release()) return 13;   // the creator's scope closes
    if (ix.release()) return 14;   // member 1
    if (ix.release()) return 15;   // member 0
    if (!ix.release()) return 16;  // member 2: the last one
    return 0;
}

// Bookkeeping self-test without a GPU (tests/test_abi.py): blocks are filed under their OWNING device and only handed to
// requests of that device; the cap is per device.  Returns 0 on success, the number of the failed check otherwise.
extern "C" int hprlp_alloc_cache_selftest(void) {
    using hprlp::BlockIndex;
    BlockIndex ix;
    char a, b, c3, d;
    const size_t MiB = size_t(1) << 20, cap = 64 * MiB;
    size_t got = 0;
    if (!ix.file(0, 8 * MiB, &a, cap)) return 1;
    if (!ix.file(1, 8 * MiB, &b, cap)) return 2;
    if (ix.take(2, 8 * MiB, &got) != nullptr) return 3;             // nothing of device 2
    if (ix.take(1, 8 * MiB, &got) != &b || got != 8 * MiB) return 4;  // device 1 gets ITS block, not device 0's
    if (ix.take(1, 8 * MiB, &got) != nullptr) return 5;             // and never device 0's
    if (ix.held(0) != 8 * MiB || ix.held(1) != 0) return 6;
    if (!ix.file(0, 40 * MiB, &c3, cap)) return 7;
    if (ix.file(0, 32 * MiB, &d, cap)) return 8;                    // over device 0's cap ...
    if (!ix.file(1, 32 * MiB, &d, cap)) return 9;                   // ... which does not count against device 1
    if (ix.take(0, 6 * MiB, &got) != &a) return 10;                 // 8 MiB block serves 6 MiB (wastes a quarter)
    if (ix.take(0, 20 * MiB, &got) != nullptr) return 11;           // the 40 MiB block would waste half of itself
    if (ix.take(0, 32 * MiB, &got) != &c3 || got != 40 * MiB) return 12;
    return 0;
}
