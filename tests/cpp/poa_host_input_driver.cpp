// poa_host_input_driver.cpp -- PoaBatch with the reads left in the pinned staging block (host input), on the CPU.
//
// Built by tests/test_poa_host_input.py from this file and the host sources under test (cudapoa_batch.cpp, runtime.cpp,
// logging.cpp, device_pool.cpp) with nothing else: every HIP entry point and every kernel-library entry point they call is a recording
// stand-in defined here, in the style of poa_host_replay_driver.cpp, so the same sources also build as one stand-alone
// program under -fsanitize=address,undefined. "Device" memory is host memory, an asynchronous copy is a memcpy, streams and
// events only record. hipHostGetDevicePointer succeeds (the device address of pinned memory is its host address) unless a
// scenario switches it off. Pinned memory is handed out filled with 0xAB, so that a slack nobody zeroed shows.
//
// The generate stand-in plays a kernel that reads args->sequences until the event behind the graph build has passed: it
// keeps a copy of the bytes it was given, and whatever later waits for that event (or for the stream) finds out whether
// the block still holds them. A block that was rewritten, or freed, under a launch in flight is a failure.
//
// The program checks itself: it prints one line per check and returns the number of failed ones.
#include <hip/hip_runtime_api.h>

#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/cudapoa/cudapoa.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gwhip.h"
#include "poa_batch_impl.hpp"

namespace
{
struct Region
{
    char* base;
    size_t bytes;
    bool device;
};
std::vector<Region> g_live;
std::vector<std::string> g_calls; // since the last take()
bool g_map_ok = true;
int g_failed  = 0;

struct Event
{
    int id;
};
std::vector<std::unique_ptr<Event>> g_events;

// the launch whose graph-build kernel may still be reading the sequences it was given
struct InFlight
{
    bool active = false;
    const uint8_t* sequences = nullptr;
    std::vector<uint8_t> bytes; // what it was given: the reads and the 2 KiB behind them
    const Event* event = nullptr;
    bool corrupted = false; // the block changed, or went away, before the launch was waited for
} g_flight;

std::string where(const void* p)
{
    if (p == nullptr) return "null";
    const char* c = static_cast<const char*>(p);
    for (const Region& r : g_live)
        if (c >= r.base && c < r.base + r.bytes) return std::string(r.device ? "dev+" : "pin+") + std::to_string(c - r.base);
    return "host";
}

void call(const std::string& text) { g_calls.push_back(text); }

std::vector<std::string> take()
{
    std::vector<std::string> out;
    out.swap(g_calls);
    return out;
}

void check(bool ok, const std::string& what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++g_failed;
}

void launch_is_over()
{
    if (!g_flight.active) return;
    if (std::memcmp(g_flight.sequences, g_flight.bytes.data(), g_flight.bytes.size()) != 0) g_flight.corrupted = true;
    g_flight.active = false;
}

hipError_t allocate(void** p, size_t bytes, bool device)
{
    *p = std::malloc(bytes ? bytes : 1);
    if (*p == nullptr) return hipErrorOutOfMemory;
    std::memset(*p, device ? 0xCD : 0xAB, bytes ? bytes : 1);
    g_live.push_back(Region{static_cast<char*>(*p), bytes, device});
    return hipSuccess;
}

hipError_t release(void* p, const char* what)
{
    call(std::string(what) + " " + where(p));
    for (size_t i = 0; i < g_live.size(); ++i)
        if (g_live[i].base == p)
        {
            const char* c = reinterpret_cast<const char*>(g_flight.sequences);
            if (g_flight.active && c >= g_live[i].base && c < g_live[i].base + g_live[i].bytes)
            {
                g_flight.corrupted = true; // freed under the kernel
                g_flight.active    = false;
            }
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
hipError_t hipHostGetDevicePointer(void** device, void* host, unsigned int)
{
    call("hipHostGetDevicePointer " + where(host));
    if (!g_map_ok) return hipErrorInvalidValue;
    *device = host;
    return hipSuccess;
}
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
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error"; }
const char* hipGetErrorName(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "hipError"; }
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attribute, int)
{
    *value = attribute == hipDeviceAttributeMultiprocessorCount ? 16 : 0;
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    const char* k = kind == hipMemcpyHostToDevice ? "H2D" : kind == hipMemcpyDeviceToHost ? "D2H" : "other";
    call(std::string("copy ") + k + " " + std::to_string(bytes) + " " + where(dst) + " <- " + where(src));
    if (bytes != 0) std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t)
{
    call("memset " + std::to_string(bytes) + " of " + std::to_string(value) + " at " + where(dst));
    if (bytes != 0) std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s)
{
    *s = reinterpret_cast<hipStream_t>(new int(0));
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return hipStreamCreate(s); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return hipStreamCreate(s); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    delete reinterpret_cast<int*>(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    call("stream sync");
    launch_is_over();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int)
{
    g_events.emplace_back(new Event{static_cast<int>(g_events.size())});
    *e = reinterpret_cast<hipEvent_t>(g_events.back().get());
    call("event create #" + std::to_string(g_events.back()->id));
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    call("event destroy #" + std::to_string(reinterpret_cast<Event*>(e)->id));
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    call("event record #" + std::to_string(reinterpret_cast<Event*>(e)->id));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    call("event sync #" + std::to_string(reinterpret_cast<Event*>(e)->id));
    if (g_flight.active && g_flight.event == reinterpret_cast<Event*>(e)) launch_is_over();
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t)
{
    *ms = 1.5f;
    return hipSuccess;
}

// ---- the kernel library's entry points ----
size_t gwhip_poa_workspace_bytes(const gwhip_poa_config* cfg, int32_t windows, uint64_t) { return static_cast<size_t>(windows) * 4096 + static_cast<size_t>(cfg->max_nodes_per_graph); }
void gwhip_poa_bytes_per_window(const gwhip_poa_config* cfg, int64_t* per_poa, int64_t* per_matrix)
{
    *per_poa    = 4096 + 3 * int64_t(cfg->max_consensus_size) + 2 * int64_t(cfg->max_sequences_per_poa) * cfg->max_sequence_size;
    *per_matrix = int64_t(cfg->matrix_sequence_dimension) * cfg->max_nodes_per_graph * 2;
}
int32_t gwhip_poa_resident_windows(const gwhip_poa_config*) { return 64; }
// as the library answers (tests/test_poa_host_input.py holds the library's own function to the same rule): the LDS-table
// kernels of the static and the adaptive band
int32_t gwhip_poa_reads_host_sequences(const gwhip_poa_config* cfg)
{
    return !cfg->size32 && cfg->max_nodes_per_graph + 2 <= 3074 && cfg->max_sequence_size + 16 <= 2048 &&
           (cfg->band_mode == GWHIP_STATIC_BAND || cfg->band_mode == GWHIP_ADAPTIVE_BAND);
}
int gwhip_last_error_string(char* buf, size_t n)
{
    if (n) buf[0] = 0;
    return 0;
}

int gwhip_poa_generate(const gwhip_poa_args* a, gwhip_stream_t stream)
{
    call("generate " + std::to_string(a->total_windows) + " windows, sequences " + where(a->sequences) + ", weights " + where(a->base_weights) +
         ", event " + (a->event_after_graph_build ? "#" + std::to_string(reinterpret_cast<Event*>(a->event_after_graph_build)->id) : std::string("none")));
    if (g_flight.active) call("GENERATE WITH A LAUNCH STILL READING ITS INPUT");
    // the extent of the reads: behind the last read of the last window
    const gwhip_window_details& last = a->window_details[a->total_windows - 1];
    size_t end                        = static_cast<size_t>(last.seq_starts);
    for (uint16_t r = 0; r < last.num_seqs; ++r) end += (static_cast<size_t>(a->sequence_lengths[last.seq_len_buffer_offset + r]) + 3) & ~size_t(3);
    bool slack_zero = true;
    for (size_t i = 0; i < 2048; ++i) slack_zero = slack_zero && a->sequences[end + i] == 0;
    call(std::string("   slack ") + (slack_zero ? "zero" : "NOT ZERO") + " behind " + std::to_string(end) + " bytes");
    g_flight.active    = true;
    g_flight.sequences = a->sequences;
    g_flight.bytes.assign(a->sequences, a->sequences + end + 2048);
    g_flight.event = reinterpret_cast<const Event*>(a->event_after_graph_build);
    // the result: every window's first read back to front, as the kernels write a consensus
    for (int32_t w = 0; w < a->total_windows; ++w)
    {
        const gwhip_window_details& wd = a->window_details[w];
        uint8_t* cons                  = a->consensus + static_cast<size_t>(w) * static_cast<size_t>(a->cfg.max_consensus_size);
        std::memset(cons, 0, static_cast<size_t>(a->cfg.max_consensus_size));
        const int32_t len = a->sequence_lengths[wd.seq_len_buffer_offset];
        for (int32_t i = 0; i < len; ++i)
        {
            cons[i] = a->sequences[static_cast<size_t>(wd.seq_starts) + static_cast<size_t>(len - 1 - i)];
            a->coverage[static_cast<size_t>(w) * static_cast<size_t>(a->cfg.max_consensus_size) + static_cast<size_t>(i)] = 1;
        }
    }
    if (a->event_after_graph_build) (void)hipEventRecord(static_cast<hipEvent_t>(a->event_after_graph_build), static_cast<hipStream_t>(stream));
    return 0;
}
int gwhip_poa_export_graphs_range(const gwhip_poa_args*, int32_t, int32_t, uint8_t*, int32_t*, uint16_t*, uint16_t*, int32_t*, uint16_t*, gwhip_stream_t) { return 0; }
} // extern "C"

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudapoa;

namespace
{
uint64_t g_rng = 77;
std::string random_read(size_t n)
{
    std::string r(n, 'A');
    for (char& c : r)
    {
        g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
        c     = "ACGT"[(g_rng >> 33) % 4];
    }
    return r;
}

// adds windows of `reads` reads of the given lengths; returns the padded bytes they take
size_t fill(Batch& batch, const std::vector<std::vector<size_t>>& windows, std::vector<std::string>* first_reads = nullptr)
{
    size_t bytes = 0;
    for (const auto& lengths : windows)
    {
        std::vector<std::string> reads;
        for (size_t n : lengths) reads.push_back(random_read(n));
        Group g;
        for (const std::string& r : reads) g.push_back(Entry{r.c_str(), nullptr, static_cast<int32_t>(r.size())});
        std::vector<StatusType> per_read;
        if (batch.add_poa_group(per_read, g) != StatusType::success) check(false, "add_poa_group");
        for (size_t n : lengths) bytes += (n + 3) & ~size_t(3);
        if (first_reads) first_reads->push_back(reads[0]);
    }
    return bytes;
}

bool has(const std::vector<std::string>& calls, const std::string& part)
{
    for (const std::string& c : calls)
        if (c.find(part) != std::string::npos) return true;
    return false;
}
size_t index_of(const std::vector<std::string>& calls, const std::string& part)
{
    for (size_t i = 0; i < calls.size(); ++i)
        if (calls[i].find(part) != std::string::npos) return i;
    return calls.size();
}
void dump(const std::vector<std::string>& calls)
{
    for (const std::string& c : calls) std::printf("      | %s\n", c.c_str());
}

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// The blocks of a BatchConfig(200, 4, ...) batch of `max_poas` windows start [sequences | weights | lengths | windows | ...],
// every array rounded up to 256 bytes (PoaBlockLayout).
struct Offsets
{
    size_t weights, lengths, windows;
    explicit Offsets(int32_t max_poas)
    {
        const size_t sequences = up256(static_cast<size_t>(max_poas) * 4 * 200 + 4096);
        weights                = sequences;
        lengths                = 2 * sequences;
        windows                = lengths + up256(static_cast<size_t>(max_poas) * 4 * sizeof(int32_t));
    }
};

// what generate_poa() did before there was host input, for n padded bytes of reads in w windows of r reads in all
std::vector<std::string> upload_path_calls(size_t n, size_t w, size_t r, const Offsets& at)
{
    return {"copy H2D " + std::to_string(n) + " dev+0 <- pin+0",
            "memset " + std::to_string(n) + " of 1 at dev+" + std::to_string(at.weights),
            "memset 2048 of 0 at dev+" + std::to_string(n),
            "copy H2D " + std::to_string(w * sizeof(gwhip_window_details)) + " dev+" + std::to_string(at.windows) + " <- pin+" + std::to_string(at.windows),
            "copy H2D " + std::to_string(4 * r) + " dev+" + std::to_string(at.lengths) + " <- pin+" + std::to_string(at.lengths),
            "generate " + std::to_string(w) + " windows, sequences dev+0, weights dev+" + std::to_string(at.weights) + ", event none",
            "   slack zero behind " + std::to_string(n) + " bytes"};
}

std::unique_ptr<Batch> make_batch(hipStream_t stream, const BatchConfig& config, int32_t windows)
{
    const gwhip_poa_config dc = make_device_config(config, OutputType::consensus, -8, -6, 8);
    int64_t per_poa = 0, per_matrix = 0;
    gwhip_poa_bytes_per_window(&dc, &per_poa, &per_matrix);
    const int64_t budget = windows * (per_poa + per_matrix) + (int64_t(1) << 20);
    DefaultDeviceAllocator allocator(static_cast<size_t>(budget), stream);
    return create_batch(0, stream, allocator, budget, OutputType::consensus, config, -8, -6, 8);
}

void fetch(Batch& batch, const std::vector<std::string>& first_reads, const char* what)
{
    std::vector<std::string> consensus;
    std::vector<std::vector<uint16_t>> coverage;
    std::vector<StatusType> status;
    batch.get_consensus(consensus, coverage, status);
    check(consensus == first_reads, std::string(what) + ": every consensus is the window's first read (the stand-in's result, read from the sequences it was given)");
}

void scenario_host_input(hipStream_t stream)
{
    std::printf("==== host input\n");
    unsetenv("GW_POA_HOST_INPUT");
    g_map_ok = true;
    const BatchConfig config(200, 4, 128, BandMode::static_band);
    {
        std::unique_ptr<Batch> batch = make_batch(stream, config, 8);
        PoaBatch& impl               = dynamic_cast<PoaBatch&>(*batch);
        const Offsets at(impl.max_poas());
        std::vector<std::string> calls = take();
        check(has(calls, "hipHostGetDevicePointer pin+0"), "the constructor asks for the device address of the pinned block");

        std::vector<std::string> firsts;
        const size_t n = fill(*batch, {{120, 117, 1}, {63}, {199, 200, 3, 64}}, &firsts);
        take();
        batch->generate_poa();
        calls = take();
        dump(calls);
        check(impl.last_generate_read_host(), "generate_poa() used host input");
        check(!has(calls, "copy H2D " + std::to_string(n) + " dev+0"), "no sequence copy");
        check(!has(calls, "memset 2048 of 0 at dev+"), "no zeroing of the device slack");
        check(has(calls, "memset " + std::to_string(n) + " of 1 at dev+" + std::to_string(at.weights)), "the unit weights are filled on the device as before");
        check(has(calls, "copy H2D " + std::to_string(3 * sizeof(gwhip_window_details))) && has(calls, "copy H2D " + std::to_string(4 * 8) + " dev+" + std::to_string(at.lengths)),
              "window details and lengths go up as before");
        check(has(calls, "generate 3 windows, sequences pin+0, weights dev+" + std::to_string(at.weights) + ", event #0"), "the launch gets the pinned address and the batch's event");
        check(has(calls, "slack zero behind " + std::to_string(n) + " bytes"), "the slack is zero in the host buffer");
        check(index_of(calls, "event record #0") == calls.size() - 1, "the event is recorded behind the graph build");
        fetch(*batch, firsts, "host input");
        check(!g_flight.active && !g_flight.corrupted, "fetching the results ended the launch with its input intact");

        // ---- relaunches: inputs resident in HBM
        take();
        impl.relaunch_resident();
        calls = take();
        dump(calls);
        check(index_of(calls, "copy H2D " + std::to_string(n) + " dev+0 <- pin+0") == 0 && index_of(calls, "memset 2048 of 0 at dev+" + std::to_string(n)) == 1,
              "the first relaunch uploads the reads once, slack zeroed");
        check(has(calls, "generate 3 windows, sequences dev+0") && has(calls, "event none"), "and launches with the device pointer");
        impl.relaunch_resident();
        calls = take();
        check(!has(calls, "dev+0 <- pin+0") && !has(calls, "memset") && has(calls, "generate 3 windows, sequences dev+0"), "the second relaunch uploads nothing");
        float a = 0, b = 0;
        impl.relaunch_resident_timed(&a, &b);
        calls = take();
        check(!has(calls, "dev+0 <- pin+0") && has(calls, "generate 3 windows, sequences dev+0"), "nor does a timed relaunch");
        check(!g_flight.corrupted, "the relaunches' input stayed intact");

        // ---- reset() behind a launch whose results nobody fetched
        batch->generate_poa();
        take();
        check(g_flight.active && where(g_flight.sequences) == "pin+0",
              "a launch is reading the pinned block");
        batch->reset();
        calls = take();
        check(calls.size() == 1 && calls[0] == "event sync #0", "reset() waits for the launch's event, and does nothing else");
        firsts.clear();
        const size_t n2 = fill(*batch, {{16, 16}, {5}}, &firsts);
        check(take().empty(), "the refill behind it needs no further wait");
        check(!g_flight.corrupted, "the block was not rewritten under the launch");
        batch->generate_poa();
        calls = take();
        check(has(calls, "generate 2 windows, sequences pin+0") && has(calls, "slack zero behind " + std::to_string(n2) + " bytes"),
              "the second fill is launched from the pinned block, slack zeroed behind its own reads");
        impl.relaunch_resident();
        calls = take();
        check(index_of(calls, "copy H2D " + std::to_string(n2) + " dev+0 <- pin+0") == 0, "a relaunch of the new fill uploads the new reads");
        fetch(*batch, firsts, "second fill");

        // ---- a refill WITHOUT reset() behind a launch: add_poa_group() appends to the block the kernel reads
        batch->generate_poa();
        take();
        check(g_flight.active, "a launch is reading the pinned block");
        const size_t n3 = n2 + fill(*batch, {{33, 31}}, &firsts);
        calls           = take();
        check(!calls.empty() && calls[0] == "event sync #0", "add_poa_group() behind a launch waits for its event first");
        check(!g_flight.corrupted, "and only then writes");
        batch->generate_poa();
        calls = take();
        check(has(calls, "generate 3 windows, sequences pin+0") && has(calls, "slack zero behind " + std::to_string(n3) + " bytes"), "the grown fill is launched");
        fetch(*batch, firsts, "grown fill");

        // ---- the switch, per call
        setenv("GW_POA_HOST_INPUT", "0", 1);
        take();
        batch->generate_poa();
        calls = take();
        dump(calls);
        check(!impl.last_generate_read_host(), "GW_POA_HOST_INPUT=0: generate_poa() uploads");
        check(calls == upload_path_calls(n3, 3, 5, at), "GW_POA_HOST_INPUT=0: the calls are the old ones, in the old order");
        impl.relaunch_resident();
        calls = take();
        check(!has(calls, "dev+0 <- pin+0"), "and a relaunch behind it uploads nothing");
        unsetenv("GW_POA_HOST_INPUT");
        batch->generate_poa();
        check(impl.last_generate_read_host(), "the switch is read per call");

        // ---- destruction with that launch in flight; the pinned cache holds nothing, so the block goes back to the system
        take();
    }
    std::vector<std::string> calls = take();
    dump(calls);
    const size_t freed = index_of(calls, "hipHostFree pin+0");
    check(freed < calls.size() && index_of(calls, "stream sync") < freed, "the destructor synchronises before the pinned block is freed");
    check(!g_flight.active && !g_flight.corrupted, "no launch was reading it by then");
}

void scenario_not_mapped(hipStream_t stream)
{
    std::printf("==== the pinned block has no device address\n");
    g_map_ok = false;
    const BatchConfig config(200, 4, 128, BandMode::static_band);
    std::unique_ptr<Batch> batch = make_batch(stream, config, 8);
    PoaBatch& impl               = dynamic_cast<PoaBatch&>(*batch);
    const Offsets at(impl.max_poas());
    const size_t n               = fill(*batch, {{120, 117, 1}, {63}});
    take();
    batch->generate_poa();
    std::vector<std::string> calls = take();
    dump(calls);
    check(calls == upload_path_calls(n, 2, 4, at), "the calls are the old ones, in the old order");
    batch->reset();
    fill(*batch, {{7}});
    check(take().empty(), "reset() and a refill wait for nothing");
    g_map_ok = true;
}

void scenario_full_band(hipStream_t stream)
{
    std::printf("==== a configuration whose kernel needs the reads in HBM\n");
    const BatchConfig config(200, 4, 128, BandMode::full_band);
    std::unique_ptr<Batch> batch = make_batch(stream, config, 8);
    PoaBatch& impl               = dynamic_cast<PoaBatch&>(*batch);
    std::vector<std::string> calls = take();
    check(!has(calls, "hipHostGetDevicePointer"), "the constructor does not ask for a device address");
    const size_t n = fill(*batch, {{100, 90}});
    take();
    batch->generate_poa();
    calls = take();
    check(!impl.last_generate_read_host() && has(calls, "copy H2D " + std::to_string(n) + " dev+0 <- pin+0") && has(calls, "sequences dev+0"), "generate_poa() uploads");
}
} // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    setenv("GW_PINNED_CACHE_BYTES", "0", 1); // a released pinned block goes back to the system at once
    Init();
    hipStream_t stream = nullptr;
    (void)hipStreamCreate(&stream);
    scenario_host_input(stream);
    scenario_not_mapped(stream);
    scenario_full_band(stream);
    (void)hipStreamDestroy(stream);
    std::printf("%d checks failed\n", g_failed);
    return g_failed == 0 ? 0 : 1;
}
