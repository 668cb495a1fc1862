// poa_host_replay_driver.cpp -- replays the cudapoa host path on the CPU: one PoaBatch through its whole life, and the two
// multi-batch drivers of cudapoa/multi_device.hpp. It prints every HIP call and every kernel-library call the host code
// makes, and every value it hands back. tests/test_poa_host_replay.py compares the text with tests/golden/poa_host_replay.txt,
// recorded from the commit before PoaBatch and the drivers were folded onto shared helpers.
//
// The executable defines recording stand-ins for the HIP runtime entry points the POA host code calls and for
// gwhip_poa_generate, gwhip_poa_export_graphs_range and gwhip_poa_resident_windows; defined here, they take precedence over
// the shared libraries' versions. gwhip_poa_workspace_bytes and gwhip_poa_bytes_per_window are the kernel library's own.
// "Device" memory is host memory, an asynchronous copy is a memcpy, streams and events only record. No address is printed:
// a pointer appears as the allocation it lies in plus its offset. The device reports 16 compute units.
//
// The generate stand-in writes a fake result per window: the first read back to front into the consensus row (as the
// kernels write it), a ramp into the coverage row, the reads into the MSA rows, the first read's length as node count into
// its length slot, and the kernel-error marker with status 4 where the first read starts with "NNNNNNNN".
//
// Scenarios: (a) sequential, full text. (b) one worker, full text. (c) four workers on a shared cursor: outputs by window
// only. (d) size classes: one thread per class, so the text is printed per stream once the call has returned, and calls
// without a stream are sorted.
#include <hip/hip_runtime_api.h>

#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/cudapoa/cudapoa.hpp>
#include <claraparabricks/genomeworks/cudapoa/multi_device.hpp>
#include <claraparabricks/genomeworks/logging/logging.hpp>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "gwhip.h"
#include "poa_batch_impl.hpp"

namespace
{
std::mutex g_mutex;
enum class Mode
{
    sequential,
    quiet,
    per_stream
};
Mode g_mode = Mode::sequential;
std::thread::id g_main_thread;

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
    std::string name;
    std::vector<std::string> lines;
};
struct Event
{
    std::string name;
};
std::vector<std::unique_ptr<Stream>> g_streams; // kept until the scenario ends: their lines are printed then
std::vector<std::unique_ptr<Event>> g_events;
std::vector<std::string> g_misc;
int g_events_created = 0;

std::string format(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

const char* name_of(hipStream_t s) { return s == nullptr ? "stream(null)" : reinterpret_cast<Stream*>(s)->name.c_str(); }

// (g_mutex held)
void line(hipStream_t s, const std::string& text)
{
    if (g_mode == Mode::quiet) return;
    if (g_mode == Mode::sequential)
        std::printf("%s\n", text.c_str());
    else if (s != nullptr)
        reinterpret_cast<Stream*>(s)->lines.push_back(text);
    else
        g_misc.push_back(text);
}

// (g_mutex held)
std::string where(const void* p)
{
    if (p == nullptr) return "null";
    const char* c = static_cast<const char*>(p);
    for (const Region& r : g_live)
        if (c >= r.base && c < r.base + r.bytes)
        {
            // (with one thread per class, which allocation comes first is a matter of timing: no number then)
            const std::string id = g_mode == Mode::sequential ? "#" + std::to_string(r.id) : "";
            return std::string(r.device ? "dev" : "pin") + id + "+" + std::to_string(c - r.base);
        }
    return "host";
}

void end_scenario()
{
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_mode == Mode::per_stream)
    {
        std::sort(g_misc.begin(), g_misc.end());
        std::printf("-- calls without a stream, sorted\n");
        for (const std::string& l : g_misc) std::printf("%s\n", l.c_str());
        for (const auto& s : g_streams)
        {
            std::printf("-- %s\n", s->name.c_str());
            for (const std::string& l : s->lines) std::printf("%s\n", l.c_str());
        }
    }
    g_misc.clear();
    g_streams.clear();
    g_events.clear();
    g_events_created = 0;
}

hipError_t allocate(void** p, size_t bytes, bool device)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    *p = std::calloc(bytes ? bytes : 1, 1);
    if (*p == nullptr) return hipErrorOutOfMemory;
    const int id = device ? g_next_device++ : g_next_pinned++;
    g_live.push_back(Region{static_cast<const char*>(*p), bytes, device, id});
    if (g_mode == Mode::sequential)
        line(nullptr, format("%s %zu -> %s#%d", device ? "hipMalloc" : "hipHostMalloc", bytes, device ? "dev" : "pin", id));
    else
        line(nullptr, format("%s %zu", device ? "hipMalloc" : "hipHostMalloc", bytes));
    return hipSuccess;
}

hipError_t release(void* p, const char* what)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(nullptr, std::string(what) + " " + where(p));
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
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error"; }
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attribute, int)
{
    *value = attribute == hipDeviceAttributeMultiprocessorCount ? 16 : 0;
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest)
{
    *least    = 1;
    *greatest = -1;
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    const char* k = kind == hipMemcpyHostToDevice ? "H2D" : kind == hipMemcpyDeviceToHost ? "D2H" : "other";
    line(s, format("hipMemcpyAsync %s %s %zu bytes %s <- %s", name_of(s), k, bytes, where(dst).c_str(), where(src).c_str()));
    if (bytes != 0) std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(s, format("hipMemsetAsync %s %zu bytes of %d at %s", name_of(s), bytes, value, where(dst).c_str()));
    if (bytes != 0) std::memset(dst, value, bytes);
    return hipSuccess;
}

static hipError_t make_stream(hipStream_t* s, const std::string& how)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    g_streams.emplace_back(new Stream{"stream#" + std::to_string(g_streams.size()), {}});
    *s = reinterpret_cast<hipStream_t>(g_streams.back().get());
    line(*s, how + " -> " + g_streams.back()->name);
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) { return make_stream(s, "hipStreamCreate"); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return make_stream(s, "hipStreamCreateWithFlags"); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int priority)
{
    return make_stream(s, "hipStreamCreateWithPriority " + std::to_string(priority));
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(s, format("hipStreamDestroy %s", name_of(s)));
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(s, format("hipStreamSynchronize %s", name_of(s)));
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(s, format("hipStreamWaitEvent %s waits for %s", name_of(s), reinterpret_cast<Event*>(e)->name.c_str()));
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int flags)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    // (an event made on a worker thread is the device pool's: which comes first is a matter of timing)
    const bool numbered = g_mode == Mode::sequential || std::this_thread::get_id() == g_main_thread;
    g_events.emplace_back(new Event{numbered ? "event#" + std::to_string(g_events_created++) : "event(of a worker)"});
    *e = reinterpret_cast<hipEvent_t>(g_events.back().get());
    if (numbered) line(nullptr, format("hipEventCreate flags %u -> %s", flags, g_events.back()->name.c_str()));
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(nullptr, format("hipEventDestroy %s", reinterpret_cast<Event*>(e)->name.c_str()));
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(s, format("hipEventRecord %s on %s", reinterpret_cast<Event*>(e)->name.c_str(), name_of(s)));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_mode == Mode::sequential) line(nullptr, format("hipEventSynchronize %s", reinterpret_cast<Event*>(e)->name.c_str()));
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; } // (how often the pool asks depends on what else is pending)
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    line(nullptr, format("hipEventElapsedTime %s .. %s", reinterpret_cast<Event*>(a)->name.c_str(), reinterpret_cast<Event*>(b)->name.c_str()));
    *ms = 1.5f;
    return hipSuccess;
}

// ---- the kernel library's entry points ----
int32_t gwhip_poa_resident_windows(const gwhip_poa_config*) { return 5; }

int gwhip_poa_generate(const gwhip_poa_args* a, gwhip_stream_t stream)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    hipStream_t s = static_cast<hipStream_t>(stream);
    line(s, format("gwhip_poa_generate on %s: %d windows, mask %d, score32 %d size32 %d trace16 %d spoa_accurate %d", name_of(s), a->total_windows,
                   a->cfg.output_mask, a->cfg.score32, a->cfg.size32, a->cfg.trace16, a->cfg.spoa_accurate));
    line(s, format("   sequences %s weights %s lengths %s windows %s", where(a->sequences).c_str(), where(a->base_weights).c_str(),
                   where(a->sequence_lengths).c_str(), where(a->window_details).c_str()));
    line(s, format("   consensus %s coverage %s msa %s cells %s counters %s workspace %s (%zu bytes)", where(a->consensus).c_str(),
                   where(a->coverage).c_str(), where(a->msa).c_str(), where(a->cells).c_str(), where(a->work_counters).c_str(),
                   where(a->workspace).c_str(), a->workspace_bytes));
    line(s, format("   event after graph build %s, phase cycles %s", a->event_after_graph_build ? reinterpret_cast<Event*>(a->event_after_graph_build)->name.c_str() : "none",
                   where(a->phase_cycles).c_str()));
    if (g_mode == Mode::sequential) line(s, format("   shared_device %d", a->shared_device));
    const size_t row = static_cast<size_t>(a->cfg.max_consensus_size), per = static_cast<size_t>(a->cfg.max_sequences_per_poa);
    for (int32_t w = 0; w < a->total_windows; ++w)
    {
        const gwhip_window_details& wd = a->window_details[w];
        line(s, format("   window %d: %d reads, first length slot %d, bases from %d, scores width %d at %llu", w, wd.num_seqs, wd.seq_len_buffer_offset,
                       wd.seq_starts, wd.scores_width, static_cast<unsigned long long>(wd.scores_offset)));
        uint8_t* cons = a->consensus + static_cast<size_t>(w) * row;
        uint16_t* cov = a->coverage + static_cast<size_t>(w) * row;
        std::memset(cons, 0, row);
        if (a->cells) a->cells[w] = 1000 + static_cast<uint64_t>(w);
        if (a->phase_cycles)
            for (int k = 0; k < 6; ++k) a->phase_cycles[static_cast<size_t>(w) * 6 + k] = static_cast<uint64_t>(100 * w + k);
        if (wd.num_seqs == 0) continue; // the slot of a window whose every read was refused
        const int32_t len  = a->sequence_lengths[wd.seq_len_buffer_offset];
        const uint8_t* read = a->sequences + wd.seq_starts;
        if (len >= 8 && std::memcmp(read, "NNNNNNNN", 8) == 0)
        {
            cons[0] = 0xFF;
            cons[1] = 4;
            continue;
        }
        for (int32_t i = 0; i < len; ++i)
        {
            cons[i] = read[len - 1 - i];
            cov[i]  = static_cast<uint16_t>(7 * w + i);
        }
        if (a->msa)
        {
            size_t at = static_cast<size_t>(wd.seq_starts);
            for (uint16_t r = 0; r < wd.num_seqs; ++r)
            {
                // (after a relaunch the first slot holds the restored length again)
                const int32_t n = a->sequence_lengths[wd.seq_len_buffer_offset + r];
                uint8_t* out    = a->msa + (static_cast<size_t>(w) * per + r) * row;
                std::memset(out, 0, row);
                std::memcpy(out, a->sequences + at, static_cast<size_t>(n));
                at += (static_cast<size_t>(n) + 3) & ~size_t(3);
            }
        }
        a->sequence_lengths[wd.seq_len_buffer_offset] = len; // the node count
    }
    if (a->work_counters && (a->work_counters[0] != 0 || a->work_counters[1] != 0)) line(s, "   THE WORK COUNTERS ARE NOT ZERO");
    return 0;
}

int gwhip_poa_export_graphs_range(const gwhip_poa_args* a, int32_t first, int32_t n, uint8_t* nodes, int32_t* edges, uint16_t* weights, uint16_t* counts,
                                  int32_t* out_edges, uint16_t* out_counts, gwhip_stream_t stream)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    hipStream_t s = static_cast<hipStream_t>(stream);
    line(s, format("gwhip_poa_export_graphs_range on %s: windows [%d, %d) of %d", name_of(s), first, first + n, a->total_windows));
    line(s, format("   nodes %s edges %s weights %s counts %s outgoing %s %s", where(nodes).c_str(), where(edges).c_str(), where(weights).c_str(),
                   where(counts).c_str(), where(out_edges).c_str(), where(out_counts).c_str()));
    // a chain over the first read: node i has the one incoming edge i-1 -> i of weight i
    const size_t mn = static_cast<size_t>(a->cfg.max_nodes_per_graph);
    for (int32_t k = 0; k < n; ++k)
    {
        const gwhip_window_details& wd = a->window_details[first + k];
        if (wd.num_seqs == 0) continue;
        const int32_t len = a->sequence_lengths[wd.seq_len_buffer_offset];
        for (int32_t i = 0; i < len; ++i)
        {
            const size_t at = static_cast<size_t>(k) * mn + static_cast<size_t>(i);
            nodes[at]       = a->sequences[wd.seq_starts + i];
            counts[at]      = i > 0 ? 1 : 0;
            edges[at * GWHIP_MAX_NODE_EDGES]   = i - 1;
            weights[at * GWHIP_MAX_NODE_EDGES] = static_cast<uint16_t>(i);
        }
    }
    return 0;
}
} // extern "C"

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudapoa;

namespace
{
uint64_t g_rng = 2024;
uint32_t next_random()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(g_rng >> 33);
}
std::string random_read(size_t n)
{
    std::string r(n, 'A');
    for (char& c : r) c = "ACGT"[next_random() % 4];
    return r;
}
std::vector<std::string> random_window(size_t reads, size_t shortest, size_t longest)
{
    std::vector<std::string> w;
    for (size_t r = 0; r < reads; ++r) w.push_back(random_read(shortest + next_random() % (longest - shortest + 1)));
    return w;
}

Group group_of(const std::vector<std::string>& window)
{
    Group g;
    for (const std::string& r : window) g.push_back(Entry{r.c_str(), nullptr, static_cast<int32_t>(r.size())});
    return g;
}

std::string digest(const std::vector<uint16_t>& v)
{
    uint64_t h = 1469598103934665603ull;
    for (uint16_t x : v) h = (h ^ x) * 1099511628211ull;
    return format("%zu values, first %d last %d, hash %016llx", v.size(), v.empty() ? -1 : v.front(), v.empty() ? -1 : v.back(), static_cast<unsigned long long>(h));
}

void print_consensus(const char* what, const std::vector<std::string>& consensus, const std::vector<std::vector<uint16_t>>& coverage,
                     const std::vector<StatusType>& status)
{
    std::printf("%s: %zu consensus, %zu coverage, %zu status\n", what, consensus.size(), coverage.size(), status.size());
    for (size_t i = 0; i < consensus.size(); ++i)
        std::printf("  [%zu] status %d consensus '%s' coverage %s\n", i, i < status.size() ? static_cast<int>(status[i]) : -1, consensus[i].c_str(),
                    i < coverage.size() ? digest(coverage[i]).c_str() : "-");
}

void print_msa(const char* what, const std::vector<std::vector<std::string>>& msa, const std::vector<StatusType>& status)
{
    std::printf("%s: %zu msa, %zu status\n", what, msa.size(), status.size());
    for (size_t i = 0; i < msa.size(); ++i)
    {
        std::printf("  [%zu] status %d, %zu rows\n", i, i < status.size() ? static_cast<int>(status[i]) : -1, msa[i].size());
        for (const std::string& row : msa[i]) std::printf("      '%s'\n", row.c_str());
    }
}

void add(Batch& batch, const char* what, const std::vector<std::string>& window)
{
    std::vector<StatusType> per_read{StatusType::generic_error}; // add_poa_group() clears it
    const StatusType st = batch.add_poa_group(per_read, group_of(window));
    std::printf("add_poa_group %s: status %d, per read", what, static_cast<int>(st));
    for (StatusType s : per_read) std::printf(" %d", static_cast<int>(s));
    std::printf(", %d in the batch\n", batch.get_total_poas());
}

void section(const char* what) { std::printf("== %s\n", what); }

// ---- (a) one PoaBatch ----
void scenario_single_batch()
{
    std::printf("==== (a) one PoaBatch\n");
    g_mode = Mode::sequential;
    const BatchConfig config(200, 4, 128, BandMode::static_band);
    const int8_t mask         = OutputType::consensus | OutputType::msa;
    const gwhip_poa_config dc = make_device_config(config, mask, -8, -6, 8);
    int64_t per_poa = 0, per_matrix = 0;
    gwhip_poa_bytes_per_window(&dc, &per_poa, &per_matrix);

    section("create_batch with a budget of zero, with one too small for a window, and with one that holds a window but not its block");
    for (int64_t budget : {int64_t(0), int64_t(4096), per_poa + per_matrix + 1024})
        try
        {
            create_batch(0, nullptr, budget, mask, config, -8, -6, 8);
            std::printf("no exception\n");
        }
        catch (const std::exception& e)
        {
            std::printf("exception: %s\n", e.what());
        }

    section("create_batch");
    hipStream_t stream = nullptr;
    (void)hipStreamCreate(&stream);
    const int64_t budget = 9 * (per_poa + per_matrix) + (int64_t(1) << 20);
    {
        DefaultDeviceAllocator allocator(static_cast<size_t>(budget), stream);
        std::unique_ptr<Batch> batch = create_batch(0, stream, allocator, budget, mask, config, -8, -6, 8);
        PoaBatch& impl               = dynamic_cast<PoaBatch&>(*batch);
        std::printf("max_poas %d, batch id %d\n", impl.max_poas(), batch->batch_id());

        section("first fill");
        add(*batch, "of four reads", random_window(4, 60, 120));
        std::vector<std::string> crowded = random_window(6, 60, 120);
        crowded[1]                       = random_read(201);
        add(*batch, "with an over-long read and two reads too many", crowded);
        add(*batch, "whose every read is over-long", {random_read(300), random_read(250)});
        add(*batch, "without reads", {});
        std::vector<std::string> failing = random_window(3, 60, 120);
        failing[0]                       = "NNNNNNNN" + failing[0];
        add(*batch, "that the kernel will fail", failing);
        int32_t added = 0;
        while (batch->get_total_poas() < impl.max_poas() && added < 64)
        {
            add(*batch, "of three reads", random_window(3, 40, 199));
            ++added;
        }
        add(*batch, "beyond the batch's capacity", random_window(3, 40, 199));

        section("generate_poa");
        batch->generate_poa();

        section("get_consensus behind one earlier result (a full batch: one copy)");
        std::vector<std::string> consensus{"earlier"};
        std::vector<std::vector<uint16_t>> coverage{{1, 2, 3}};
        std::vector<StatusType> status{StatusType::generic_error};
        std::printf("returns %d\n", static_cast<int>(batch->get_consensus(consensus, coverage, status)));
        print_consensus("get_consensus", consensus, coverage, status);

        section("get_consensus_in_place over those vectors");
        std::printf("returns %d\n", static_cast<int>(impl.get_consensus_in_place(consensus, coverage, status)));
        print_consensus("get_consensus_in_place", consensus, coverage, status);

        section("get_msa behind one earlier result");
        std::vector<std::vector<std::string>> msa{{"earlier"}};
        status.assign(1, StatusType::generic_error);
        std::printf("returns %d\n", static_cast<int>(batch->get_msa(msa, status)));
        print_msa("get_msa", msa, status);

        section("relaunch_resident");
        impl.relaunch_resident();
        section("relaunch_resident_timed");
        float graph_ms = 0, output_ms = 0;
        impl.relaunch_resident_timed(&graph_ms, &output_ms);
        std::printf("graph build %.2f ms, output %.2f ms\n", graph_ms, output_ms);
        section("profile_phases");
        double phases[6];
        impl.profile_phases(phases);
        std::printf("phases %.3f %.3f %.3f %.3f %.3f %.3f\n", phases[0], phases[1], phases[2], phases[3], phases[4], phases[5]);

        section("get_graphs in two chunks");
        const size_t per_window = static_cast<size_t>(config.max_nodes_per_graph) * (1 + 2 + GWHIP_MAX_NODE_EDGES * (4 + 2)) + 4 * 256;
        setenv("GW_GRAPH_EXPORT_CHUNK_BYTES", std::to_string(per_window * static_cast<size_t>((batch->get_total_poas() + 1) / 2)).c_str(), 1);
        std::vector<DirectedGraph> graphs;
        status.assign(1, StatusType::generic_error);
        batch->get_graphs(graphs, status);
        unsetenv("GW_GRAPH_EXPORT_CHUNK_BYTES");
        std::printf("%zu graphs, status", graphs.size());
        for (StatusType s : status) std::printf(" %d", static_cast<int>(s));
        std::printf("\n");
        for (size_t i = 0; i < graphs.size(); ++i)
        {
            std::string labels;
            for (int32_t n = 0; !graphs[i].get_node_label(n).empty(); ++n) labels += graphs[i].get_node_label(n);
            uint64_t h = 1469598103934665603ull;
            const auto edges = graphs[i].get_edges();
            for (const auto& e : edges) h = (((h ^ static_cast<uint64_t>(e.first.first)) * 1099511628211ull ^ static_cast<uint64_t>(e.first.second)) * 1099511628211ull ^ static_cast<uint64_t>(e.second)) * 1099511628211ull;
            std::printf("  [%zu] nodes '%s', %zu edges, hash %016llx\n", i, labels.c_str(), edges.size(), static_cast<unsigned long long>(h));
        }

        section("total_cells");
        std::printf("total_cells %llu\n", static_cast<unsigned long long>(impl.total_cells()));

        section("reset and a second fill of two windows");
        batch->reset();
        std::printf("%d in the batch\n", batch->get_total_poas());
        section("generate_poa on the empty batch");
        batch->generate_poa();
        add(*batch, "of four reads", random_window(4, 150, 200));
        add(*batch, "of two reads", random_window(2, 30, 60));
        section("generate_poa");
        batch->generate_poa();
        section("get_consensus into empty vectors (a batch that is mostly empty: two copies)");
        consensus.clear();
        coverage.clear();
        status.clear();
        std::printf("returns %d\n", static_cast<int>(batch->get_consensus(consensus, coverage, status)));
        print_consensus("get_consensus", consensus, coverage, status);
        section("total_cells");
        std::printf("total_cells %llu\n", static_cast<unsigned long long>(impl.total_cells()));

        section("destroy");
    }
    section("a consensus-only batch refuses get_msa, an msa-only batch get_consensus");
    for (int8_t one : {static_cast<int8_t>(OutputType::consensus), static_cast<int8_t>(OutputType::msa)})
    {
        DefaultDeviceAllocator allocator(static_cast<size_t>(budget), stream);
        std::unique_ptr<Batch> batch = create_batch(0, stream, allocator, budget, one, config, -8, -6, 8);
        std::vector<std::string> consensus;
        std::vector<std::vector<uint16_t>> coverage;
        std::vector<std::vector<std::string>> msa;
        std::vector<StatusType> status;
        add(*batch, "of three reads", random_window(3, 40, 100));
        batch->generate_poa();
        std::printf("get_consensus returns %d\n", static_cast<int>(batch->get_consensus(consensus, coverage, status)));
        std::printf("get_msa returns %d\n", static_cast<int>(batch->get_msa(msa, status)));
        print_consensus("get_consensus", consensus, coverage, status);
        print_msa("get_msa", msa, status);
    }
    (void)hipStreamDestroy(stream);
    end_scenario();
}

// ---- the multi-batch drivers ----
void print_output(const MultiDeviceOutput& out, int32_t workers, bool deterministic_workers)
{
    bool in_range = true;
    for (int32_t w : out.worker_of_window) in_range = in_range && w >= -1 && w < workers;
    std::printf("%zu windows, workers in range: %s, seconds >= 0: %s, seconds_after_creation >= 0: %s\n", out.status.size(), in_range ? "yes" : "NO",
                out.seconds >= 0 ? "yes" : "NO", out.seconds_after_creation >= 0 ? "yes" : "NO");
    for (size_t w = 0; w < out.status.size(); ++w)
    {
        std::printf("  window %zu: status %d", w, static_cast<int>(out.status[w]));
        if (deterministic_workers) std::printf(" worker %d", out.worker_of_window[w]);
        if (!out.consensus.empty()) std::printf(" consensus '%s' coverage %s", out.consensus[w].c_str(), digest(out.coverage[w]).c_str());
        std::printf("\n");
        if (!out.msa.empty())
            for (const std::string& row : out.msa[w]) std::printf("      '%s'\n", row.c_str());
    }
}

std::vector<std::vector<std::string>> shared_cursor_windows()
{
    std::vector<std::vector<std::string>> windows;
    for (int w = 0; w < 13; ++w) windows.push_back(random_window(2 + static_cast<size_t>(w) % 3, 40, 190));
    windows[3]  = {random_read(400)};                  // its only read is over-long: the slot of an empty POA
    windows[7]  = {};                                  // no reads: no slot
    windows[9][1] = random_read(201);                  // one read refused
    return windows;
}

void scenario_one_worker()
{
    std::printf("==== (b) process_windows_multi_device with one worker\n");
    g_mode = Mode::sequential;
    const BatchConfig config(200, 4, 128, BandMode::static_band);
    const std::vector<std::vector<std::string>> windows = shared_cursor_windows();
    for (int run = 0; run < 4; ++run)
    {
        MultiDeviceConfig mc;
        mc.memory_per_device = int64_t(48) << 20;
        mc.output_mask       = run == 1 ? OutputType::msa : OutputType::consensus;
        if (run == 2) setenv("GW_POA_FILL_ROUNDS", "0", 1);
        section(run == 0 ? "consensus, fills of one device round" : run == 1 ? "msa" : run == 2 ? "consensus with GW_POA_FILL_ROUNDS=0" : "no windows");
        MultiDeviceOutput out;
        process_windows_multi_device(out, run == 3 ? std::vector<std::vector<std::string>>() : windows, config, mc);
        unsetenv("GW_POA_FILL_ROUNDS");
        std::printf("launches %d\n", out.launches);
        print_output(out, 1, true);
        end_scenario();
    }
    section("a batch too small for a window");
    try
    {
        MultiDeviceConfig mc;
        mc.memory_per_device = int64_t(1) << 16;
        MultiDeviceOutput out;
        process_windows_multi_device(out, windows, config, mc);
        std::printf("no exception\n");
    }
    catch (const std::exception& e)
    {
        std::printf("exception: %s\n", e.what());
    }
    end_scenario();
}

void scenario_four_workers()
{
    std::printf("==== (c) process_windows_multi_device with devices (0, 0) x 2 batches\n");
    g_mode = Mode::quiet;
    const BatchConfig config(200, 4, 128, BandMode::static_band);
    std::vector<std::vector<std::string>> windows = shared_cursor_windows();
    for (int w = 0; w < 40; ++w) windows.push_back(random_window(3, 40, 190));
    MultiDeviceConfig mc;
    mc.devices           = {0, 0};
    mc.batches_per_device = 2;
    mc.memory_per_device = int64_t(96) << 20;
    MultiDeviceOutput out;
    process_windows_multi_device(out, windows, config, mc);
    // every launch holds at most one device round (five windows, gwhip_poa_resident_windows above), whoever takes which
    // window; 52 of the 53 windows own a slot
    const int32_t floor = (52 + 4) / 5;
    std::printf("launches >= %d: %s\n", floor, out.launches >= floor ? "yes" : "NO");
    print_output(out, 4, false);
    end_scenario();
}

void scenario_size_classes()
{
    std::printf("==== (d) process_windows_size_classes\n");
    // three classes by longest read: (500, 1000], (250, 500], (125, 250]; full band, so the first class's windows are large
    // and, under the budget below, its 12 windows need a second fill; 12 + 4 fit the 20 windows the 16 compute units admit, the third class is gated
    std::vector<std::vector<std::string>> windows;
    for (int w = 0; w < 12; ++w) windows.push_back(random_window(2 + static_cast<size_t>(w) % 2, 600, 1000));
    for (int w = 0; w < 4; ++w) windows.push_back(random_window(3, 300, 500));
    for (int w = 0; w < 6; ++w) windows.push_back(random_window(3, 130, 250));
    windows[0][0] = random_read(1000);
    windows[14]   = {random_read(600)}; // over-long for its class (below): the slot of an empty POA
    std::vector<int32_t> longest, reads;
    for (const auto& w : windows)
    {
        size_t l = 0;
        for (const std::string& r : w) l = std::max(l, r.size());
        longest.push_back(static_cast<int32_t>(l));
        reads.push_back(static_cast<int32_t>(w.size()));
    }
    longest[14] = 400;
    SizeClassPlan plan;
    plan_size_classes(plan, longest, reads, false, 128, BandMode::full_band);
    std::printf("%zu classes:", plan.configs.size());
    for (size_t k = 0; k < plan.configs.size(); ++k) std::printf(" %zu windows of up to %d bases,", plan.groups[k].size(), plan.configs[k].max_sequence_size);
    const std::vector<int32_t> gates = size_class_admission_gates(plan, 16);
    std::printf(" gates");
    for (int32_t g : gates) std::printf(" %d", g);
    std::printf("\n");

    for (int run = 0; run < 3; ++run)
    {
        g_mode = Mode::per_stream;
        section(run == 0 ? "consensus" : run == 1 ? "msa" : "with a class whose share does not hold its batch in front, and a class without reads behind");
        SizeClassPlan p = plan;
        if (run == 2)
        {
            // a class of 16000-base full-band windows whose plan understates them: the share holds no window, create_batch throws
            p.configs.insert(p.configs.begin(), BatchConfig(16000, 2, 128, BandMode::full_band));
            p.groups.insert(p.groups.begin(), std::vector<int32_t>{static_cast<int32_t>(windows.size())});
            p.bytes_per_window.insert(p.bytes_per_window.begin(), int64_t(1) << 20);
            windows.push_back({random_read(100), random_read(90)});
            // and a fifth whose only window has no reads: its one fill leaves the batch empty, the event is recorded all the same
            p.configs.push_back(p.configs.back());
            p.groups.push_back(std::vector<int32_t>{static_cast<int32_t>(windows.size())});
            p.bytes_per_window.push_back(p.bytes_per_window.back());
            windows.push_back({});
        }
        MultiDeviceOutput out;
        double compute_seconds = -1;
        try
        {
            // (a budget that leaves every class little more than its slack: the first class holds eight of its twelve windows)
            process_windows_size_classes(out, windows, p, 0, int64_t(200) << 20, run == 1 ? OutputType::msa : OutputType::consensus, -8, -6, 8, &compute_seconds);
            std::printf("no exception\n");
        }
        catch (const std::exception& e)
        {
            std::printf("exception: %s\n", e.what());
        }
        std::printf("launches %d, compute_seconds >= 0: %s\n", out.launches, compute_seconds >= 0 ? "yes" : "NO");
        print_output(out, static_cast<int32_t>(p.configs.size()), true);
        end_scenario();
    }
    section("no windows");
    MultiDeviceOutput out;
    process_windows_size_classes(out, {}, plan, 0, int64_t(8) << 30, OutputType::consensus);
    print_output(out, 3, true);
    end_scenario();
}
} // namespace

int main(int argc, char** argv)
{
    g_main_thread = std::this_thread::get_id();
    // the library's warnings (failed windows) go to stderr: into the same text, in order
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    dup2(1, 2);
    for (const char* name : {"GW_SPOA_ACCURATE", "GW_GRAPH_EXPORT_CHUNK_BYTES", "GW_POA_FILL_ROUNDS", "GW_SIZE_CLASS_TRACE", "GW_PINNED_CACHE_BYTES"}) unsetenv(name);
    Init();
    const std::string only = argc > 1 ? argv[1] : "abcd";
    if (only.find('a') != std::string::npos) scenario_single_batch();
    if (only.find('b') != std::string::npos) scenario_one_worker();
    if (only.find('c') != std::string::npos) scenario_four_workers();
    if (only.find('d') != std::string::npos) scenario_size_classes();
    return 0;
}
