// banded_pipeline_replay_driver.cpp -- replays the banded aligner's three-stream pipeline on the CPU and prints every HIP
// call it makes, in order: which stream (own / upload / side), which copy (bytes, where from, where to), which event is
// recorded and waited for. tests/test_alignment_impl.py compares the text with tests/golden/banded_pipeline_calls.txt,
// recorded once from the commit before the host classes were refactored: any reordering of the submissions shows.
//
// The executable defines recording stand-ins for the HIP runtime entry points the host library calls and for the kernel
// entry points of the banded aligner; defined here, they take precedence over the shared libraries' versions. "Device"
// memory is host memory, an asynchronous copy is a memcpy, streams and events only record. No address is printed: a
// pointer appears as the allocation it lies in (dev#k / pin#k, numbered in order of allocation) plus its offset.
//
//   banded_pipeline_replay_driver                  the three shapes of the golden file
//   banded_pipeline_replay_driver --fail-alloc     the second chunk's workspace does not fit: align_all() throws
//   banded_pipeline_replay_driver --fail-memcpy    the second chunk's first upload returns an error (the library aborts)
#include <hip/hip_runtime_api.h>

#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "aligner_impl.hpp"
#include "gwhip.h"

namespace
{
std::mutex g_mutex;

struct Region
{
    const char* base;
    size_t bytes;
    bool device;
    int id;
};
std::vector<Region> g_live;
int g_next_device = 0, g_next_pinned = 0;

struct Stream
{
    std::string role;
};
struct Event
{
    std::string label = "unrecorded";
    int call         = -1; ///< the top-level call that recorded it last
};
int g_streams_created = 0;
Event* g_last_created = nullptr;

// per top-level call (align_all, relaunch, ...)
int g_call = 0, g_chunks = 1, g_upload_records = 0, g_side_records = 0, g_own_records = 0, g_upload_copies = 0;
bool g_fail_memcpy = false, g_fail_alloc = false;
int g_sized_calls = 0;

// While the aligner is destroyed, the order of the calls matters per stream only (a stream is synchronised, then destroyed):
// the lines of that section are held back and printed stream by stream.
bool g_destroying = false;
std::vector<std::string> g_held[3]; // own, upload, side
void flush_held()
{
    for (std::vector<std::string>& lines : g_held)
    {
        for (const std::string& line : lines) std::printf("%s\n", line.c_str());
        lines.clear();
    }
}
void stream_line(const char* call, const std::string& on)
{
    const std::string line = std::string(call) + " " + on;
    if (g_destroying && (on == "own" || on == "upload" || on == "side"))
        g_held[on == "own" ? 0 : on == "upload" ? 1 : 2].push_back(line);
    else
        std::printf("%s\n", line.c_str());
}

void begin_call(const char* what)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    flush_held();
    ++g_call;
    g_upload_records = g_side_records = g_own_records = g_upload_copies = g_sized_calls = 0;
    std::printf("== %s\n", what);
}

std::string where(const void* p)
{
    if (p == nullptr) return "null";
    const char* c = static_cast<const char*>(p);
    for (const Region& r : g_live)
        if (c >= r.base && c < r.base + r.bytes) return std::string(r.device ? "dev#" : "pin#") + std::to_string(r.id) + "+" + std::to_string(c - r.base);
    return "host";
}

const char* role(hipStream_t s) { return s == nullptr ? "own" : reinterpret_cast<Stream*>(s)->role.c_str(); }

hipError_t allocate(void** p, size_t bytes, bool device)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    *p = std::calloc(bytes ? bytes : 1, 1);
    if (*p == nullptr) return hipErrorOutOfMemory;
    const int id = device ? g_next_device++ : g_next_pinned++;
    g_live.push_back(Region{static_cast<const char*>(*p), bytes, device, id});
    std::printf("%s %zu -> %s#%d\n", device ? "hipMalloc" : "hipHostMalloc", bytes, device ? "dev" : "pin", id);
    return hipSuccess;
}

hipError_t release(void* p, const char* what)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    flush_held();
    std::printf("%s %s\n", what, where(p).c_str());
    for (size_t i = 0; i < g_live.size(); ++i)
        if (g_live[i].base == p)
        {
            g_live.erase(g_live.begin() + static_cast<long>(i));
            break;
        }
    std::free(p);
    return hipSuccess;
}
} // namespace

extern "C"
{
hipError_t hipMalloc(void** p, size_t bytes) { return allocate(p, bytes, true); }
hipError_t hipFree(void* p) { return release(p, "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return allocate(p, bytes, false); }
hipError_t hipHostFree(void* p) { return release(p, "hipHostFree"); }
hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total)
{
    *free_bytes = *total = size_t(1) << 30;
    return hipSuccess;
}
hipError_t hipGetDevice(int* device)
{
    *device = 0;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int* n)
{
    *n = 1;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error injected by the replay driver"; }

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const char* k = kind == hipMemcpyHostToDevice ? "H2D" : kind == hipMemcpyDeviceToHost ? "D2H" : "other";
    std::printf("hipMemcpyAsync %s %s %zu bytes %s <- %s\n", role(s), k, bytes, where(dst).c_str(), where(src).c_str());
    if (std::strcmp(role(s), "upload") == 0 && ++g_upload_copies == 4 && g_fail_memcpy) // three copies per chunk: the second chunk's first
    {
        std::printf("   (returns an error)\n");
        std::fflush(stdout);
        return hipErrorInvalidValue;
    }
    if (bytes != 0) std::memcpy(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    // the aligner creates its upload stream first, then its side stream; gwhip_myers_banded below checks the second name
    Stream* made = new Stream{g_streams_created == 0 ? "upload" : g_streams_created == 1 ? "side" : "stream#" + std::to_string(g_streams_created)};
    ++g_streams_created;
    std::printf("hipStreamCreateWithFlags -> %s\n", made->role.c_str());
    *s = reinterpret_cast<hipStream_t>(made);
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    stream_line("hipStreamDestroy", role(s));
    delete reinterpret_cast<Stream*>(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    stream_line("hipStreamSynchronize", role(s));
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    g_last_created = new Event;
    std::printf("hipEventCreate\n");
    *e = reinterpret_cast<hipEvent_t>(g_last_created);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    Event* ev = reinterpret_cast<Event*>(e);
    flush_held();
    // (the aligner's own events are destroyed with it, in whatever order it keeps them: only their number is printed)
    std::printf("hipEventDestroy %s\n", ev->label == "pool_free" ? "pool_free" : "(of the aligner)");
    if (g_last_created == ev) g_last_created = nullptr;
    delete ev;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    Event* ev            = reinterpret_cast<Event*>(e);
    const std::string on = role(s);
    // an event's role is read off its use: the device pool records a fresh event when it takes a block back; the upload stream
    // records "chunk k is up"; the side stream "chunk k is sized", n_chunks times, then "the side stream has joined"; the
    // aligner's own stream "the round begins"
    if (ev == g_last_created)
        ev->label = "pool_free";
    else if (on == "upload")
        ev->label = "uploaded[" + std::to_string(g_upload_records++) + "]";
    else if (on == "side")
    {
        const int k = g_side_records++;
        ev->label   = k < g_chunks ? "sized[" + std::to_string(k) + "]" : k == g_chunks ? "side_joined" : "side#" + std::to_string(k);
    }
    else
        ev->label = g_own_records++ == 0 ? "begin" : "begin#" + std::to_string(g_own_records - 1);
    ev->call       = g_call;
    g_last_created = nullptr;
    std::printf("hipEventRecord %s on %s\n", ev->label.c_str(), on.c_str());
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const Event* ev = reinterpret_cast<Event*>(e);
    std::printf("hipStreamWaitEvent %s waits for %s%s\n", role(s), ev->label.c_str(), ev->call == g_call ? "" : " (of an earlier call)");
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    std::printf("hipEventSynchronize %s\n", reinterpret_cast<Event*>(e)->label.c_str());
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    std::printf("hipEventQuery %s\n", reinterpret_cast<Event*>(e)->label.c_str());
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t)
{
    *ms = 0.f;
    return hipSuccess;
}

// ---- the kernels' entry points ----
size_t gwhip_myers_banded_workspace_bytes(int32_t, const int64_t*, const int32_t*) { return 65536; }
size_t gwhip_myers_banded_workspace_bytes_of_words(int32_t n_alignments, int64_t, int64_t)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_fail_alloc && ++g_sized_calls == 2) return size_t(1) << 40; // more than the pool holds
    return 4096 + 256 * static_cast<size_t>(n_alignments);
}
int gwhip_unpack_bases(const uint8_t* packed, char* sequences, int64_t first, int64_t last, gwhip_stream_t stream)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    std::printf("gwhip_unpack_bases %s bases [%lld, %lld) %s <- %s\n", role(static_cast<hipStream_t>(stream)), static_cast<long long>(first),
                static_cast<long long>(last), where(sequences).c_str(), where(packed).c_str());
    return 0;
}
int gwhip_myers_banded(const gwhip_myers_args* a, gwhip_stream_t stream)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const char* phase = a->phases == GWHIP_MYERS_SIZING ? "sizing" : a->phases == GWHIP_MYERS_ALIGN ? "align" : "whole";
    std::printf("gwhip_myers_banded %s on %s, side stream %s: pairs [%d, %d) bases [%lld, +%lld) capacity %lld hints %d %d\n", phase,
                role(static_cast<hipStream_t>(stream)), a->side_stream == nullptr ? "none" : role(static_cast<hipStream_t>(a->side_stream)),
                a->index_base, a->index_base + a->n_alignments, static_cast<long long>(a->first_sequence_offset),
                static_cast<long long>(a->total_sequence_length), static_cast<long long>(a->results_capacity), a->max_query_length, a->max_bandwidth_hint);
    std::printf("   sequences %s starts %s bandwidths %s order %s cells %s\n", where(a->sequences).c_str(), where(a->sequence_starts).c_str(),
                where(a->max_bandwidths).c_str(), where(a->scheduling_index).c_str(), where(a->band_cells).c_str());
    std::printf("   results %s counts %s result_starts %s metadata %s starts_base %s workspace %s (%zu bytes)\n", where(a->results).c_str(),
                where(a->result_counts).c_str(), where(a->result_starts).c_str(), where(a->result_metadata).c_str(), where(a->result_starts_base).c_str(),
                where(a->workspace).c_str(), a->workspace_bytes);
    std::printf("   on the host: results %s counts %s (%lld runs) result_starts %s metadata %s\n", where(a->results_host).c_str(),
                where(a->result_counts_host).c_str(), static_cast<long long>(a->results_host_capacity), where(a->result_starts_host).c_str(),
                where(a->result_metadata_host).c_str());
    if (a->phases == GWHIP_MYERS_SIZING) return 0;
    // no pair has a run: the offsets and the head are zeros
    const size_t n = static_cast<size_t>(a->n_alignments);
    std::memset(a->result_starts, 0, (n + 1) * 4);
    std::memset(a->result_metadata, 0, n * 4);
    if (a->result_starts_host != nullptr) std::memset(a->result_starts_host, 0, (n + 1) * 4);
    if (a->result_metadata_host != nullptr) std::memset(a->result_metadata_host, 0, n * 4);
    return 0;
}
} // extern "C"

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudaaligner;

namespace
{
constexpr int kPairs = 640;

std::vector<std::pair<std::string, std::string>> make_pairs()
{
    std::vector<std::pair<std::string, std::string>> pairs;
    uint64_t state = 12345;
    auto next      = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(state >> 33); };
    for (int k = 0; k < kPairs; ++k)
    {
        const size_t n = 40 + next() % 261; // 40 .. 300 bases
        std::string q(n, 'A');
        for (char& c : q) c = "ACGT"[next() % 4];
        std::string t = q;
        t[next() % n] = 'N';
        if (k % 3 == 0) t.erase(next() % n, 1);
        pairs.emplace_back(std::move(q), std::move(t));
    }
    return pairs;
}

void set_chunks(int chunks)
{
    if (chunks == 0)
        unsetenv("GW_ALIGNER_CHUNKS");
    else
        setenv("GW_ALIGNER_CHUNKS", std::to_string(chunks).c_str(), 1);
    g_chunks = chunks == 0 ? 1 : chunks;
}

void report_device(const Aligner& aligner, const char* when)
{
    const DeviceAlignmentsPtrs d = aligner.get_alignments_device();
    std::printf("get_alignments_device %s: %d alignments, %lld runs, operations %s offsets %s\n", when, d.n_alignments, static_cast<long long>(d.total_length),
                where(d.cigar_operations).c_str(), where(d.cigar_offsets).c_str());
}

void run_batch(FixedBandAligner& aligner, const std::vector<std::pair<std::string, std::string>>& pairs, int chunks)
{
    set_chunks(chunks);
    begin_call("add_alignment x 640");
    for (const auto& p : pairs)
        if (aligner.add_alignment(p.first.c_str(), static_cast<int32_t>(p.first.size()), p.second.c_str(), static_cast<int32_t>(p.second.size())) != StatusType::success)
            std::printf("add_alignment refused a pair\n");
    begin_call("align_all");
    if (aligner.align_all() != StatusType::success) std::printf("align_all failed\n");
    report_device(aligner, "after align_all");
    begin_call("relaunch_resident");
    dynamic_cast<BandedAligner&>(aligner).relaunch_resident();
    begin_call("sync_alignments");
    if (aligner.sync_alignments() != StatusType::success) std::printf("sync_alignments failed\n");
    report_device(aligner, "after sync_alignments");
    const auto& alignments = aligner.get_alignments();
    size_t with_result     = 0;
    for (const auto& a : alignments) with_result += a->get_status() == StatusType::success;
    std::printf("%zu alignments, %zu with a result, %d queued\n", alignments.size(), with_result, aligner.num_alignments());
}

void run_shape(const char* name, int chunks, const char* mirror_runs, int second_chunks)
{
    std::printf("==== %s\n", name);
    g_streams_created = 0;
    if (mirror_runs == nullptr)
        unsetenv("GW_ALIGNER_MIRROR_RUNS");
    else
        setenv("GW_ALIGNER_MIRROR_RUNS", mirror_runs, 1);
    const auto pairs = make_pairs();
    begin_call("create_aligner");
    std::unique_ptr<FixedBandAligner> aligner = create_aligner(AlignmentType::global_alignment, 512, nullptr, 0, int64_t(64) << 20);
    try
    {
        run_batch(*aligner, pairs, chunks);
        run_batch(*aligner, pairs, second_chunks);
    }
    catch (const std::exception& e)
    {
        // (--fail-alloc) the object must be usable again: a smaller question on the same object
        std::printf("exception: %s\n", e.what());
        g_fail_alloc = false;
        begin_call("reset after the exception");
        aligner->reset();
        run_batch(*aligner, pairs, second_chunks);
    }
    begin_call("reset");
    aligner->reset();
    begin_call("destroy");
    g_destroying = true;
    aligner.reset();
    g_destroying = false;
    flush_held();
}
} // namespace

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i)
    {
        g_fail_alloc |= std::strcmp(argv[i], "--fail-alloc") == 0;
        g_fail_memcpy |= std::strcmp(argv[i], "--fail-memcpy") == 0;
    }
    unsetenv("GW_ALIGNER_RAW_UPLOAD");
    unsetenv("GW_ALIGNER_TRACE");
    if (g_fail_alloc || g_fail_memcpy)
    {
        run_shape("GW_ALIGNER_CHUNKS=5 with a failure in the second chunk", 5, nullptr, 7);
        return 0;
    }
    run_shape("GW_ALIGNER_CHUNKS unset", 0, nullptr, 5);
    run_shape("GW_ALIGNER_CHUNKS=5", 5, nullptr, 7);
    run_shape("GW_ALIGNER_CHUNKS=7 GW_ALIGNER_MIRROR_RUNS=3", 7, "3", 5);
    return 0;
}
