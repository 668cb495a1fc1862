// multi_device.cpp -- see include/claraparabricks/genomeworks/cudapoa/multi_device.hpp.
#include <claraparabricks/genomeworks/cudapoa/multi_device.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>
#include <claraparabricks/genomeworks/utils/cudautils.hpp>
#include <claraparabricks/genomeworks/utils/signed_integer_utils.hpp>

#include "../../include/gwhip.h"
#include "owned_hip.hpp"
#include "poa_batch_impl.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <exception>
#include <map>
#include <mutex>
#include <stdexcept>
#include <thread>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapoa
{

namespace
{
using gwhost::JoinAll;
using gwhost::OwnedEvents;
using gwhost::OwnedStreams;
using Clock = std::chrono::steady_clock;

// Every worker arrives once (a second arrive() of the same worker returns at once) and leaves when all have arrived, or when
// the spawn was abandoned: a worker thread that could not be started is not waited for. The last arrival stamps the time.
struct Rendezvous
{
    Rendezvous(size_t workers, size_t expected_arrivals, const std::atomic<bool>& spawn_abandoned)
        : expected(static_cast<int32_t>(expected_arrivals))
        , abandoned(spawn_abandoned)
        , seen(workers, 0)
    {
    }
    void arrive(size_t worker)
    {
        if (seen[worker]) return;
        seen[worker] = 1;
        if (arrived.fetch_add(1) + 1 == expected) all_arrived = Clock::now(); // (read once the workers have been joined)
        while (arrived.load() < expected && !abandoned.load()) std::this_thread::yield();
    }
    bool complete() const { return arrived.load() == expected; }

    const int32_t expected;
    const std::atomic<bool>& abandoned;
    std::vector<char> seen; // [worker], touched by that worker only
    std::atomic<int32_t> arrived{0};
    Clock::time_point all_arrived{};
};

// The moment the last worker had stored its last results (before its Batch is destroyed), relative to `begin`.
struct ResultClock
{
    Clock::time_point begin{};
    std::atomic<int64_t> ns{0};
    void stamp()
    {
        const int64_t now_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - begin).count();
        int64_t seen         = ns.load();
        while (seen < now_ns && !ns.compare_exchange_weak(seen, now_ns)) {}
    }
    bool stamped() const { return ns.load() > 0; }
    Clock::time_point last() const { return begin + std::chrono::nanoseconds(ns.load()); }
};

void prepare_output(MultiDeviceOutput& out, size_t n, bool want_msa)
{
    out = MultiDeviceOutput{};
    out.status.assign(n, StatusType::success);
    out.worker_of_window.assign(n, -1);
    if (want_msa)
        out.msa.resize(n);
    else
    {
        out.consensus.resize(n);
        out.coverage.resize(n);
    }
}

// Window indices still to be taken: order[next ..), or next .. size in ascending order without one.
struct WindowQueue
{
    const std::vector<int32_t>* order = nullptr;
    size_t size                       = 0;
    size_t next                       = 0;
    bool empty() const { return next >= size; }
    size_t front() const { return order ? static_cast<size_t>((*order)[next]) : next; }
};

using WindowWeights = std::vector<std::vector<std::vector<int8_t>>>; // [window][read][base]; an empty read: unit weights

// Moves windows from the queue into the batch until it is full, holds fill_cap windows, or the queue is empty. in_batch gets
// the global index of every output slot of the launch, windows.size() for a placeholder slot; refusals go to out.status.
// weights: nullptr, or the checked weights of a weighted call (check_weights), whose refused windows are passed over.
void fill_batch(Batch& batch, std::vector<size_t>& in_batch, WindowQueue& queue, int32_t fill_cap, const std::vector<std::vector<std::string>>& windows,
                int32_t worker, MultiDeviceOutput& out, const char* holds_no_window, const WindowWeights* weights = nullptr)
{
    while (!queue.empty() && batch.get_total_poas() < fill_cap)
    {
        const size_t w                         = queue.front();
        const std::vector<std::string>& window = windows[w];
        if (weights != nullptr && out.status[w] != StatusType::success) // refused by check_weights: it takes no slot
        {
            out.worker_of_window[w] = worker;
            queue.next++;
            continue;
        }
        Group group;
        group.reserve(window.size());
        for (size_t r = 0; r < window.size(); r++)
        {
            const int8_t* of_read = weights != nullptr && !(*weights)[w][r].empty() ? (*weights)[w][r].data() : nullptr;
            group.push_back(Entry{window[r].c_str(), of_read, get_size<int32_t>(window[r])});
        }
        std::vector<StatusType> per_read;
        const StatusType st = batch.add_poa_group(per_read, group);
        if (st == StatusType::exceeded_maximum_poas)
        {
            if (in_batch.empty()) throw std::runtime_error(holds_no_window);
            break;
        }
        out.worker_of_window[w] = worker;
        if (st == StatusType::success)
            in_batch.push_back(w);
        else
        {
            out.status[w] = st;
            // every read was refused after the batch opened a POA for the group (cudapoa_batch.cuh:122-150): the empty POA
            // owns an output slot of this launch; its window reports the add status
            if (st == StatusType::empty_poa_group && !window.empty()) in_batch.push_back(windows.size());
        }
        queue.next++;
    }
}

// get_msa() or get_consensus() of the launch, stored by global window index (placeholder slots are skipped).
void store_results(Batch& batch, bool want_msa, const std::vector<size_t>& in_batch, MultiDeviceOutput& out)
{
    const size_t n = out.status.size();
    std::vector<StatusType> status;
    std::vector<std::vector<std::string>> msa;
    std::vector<std::string> consensus;
    std::vector<std::vector<uint16_t>> coverage;
    if (want_msa)
    {
        batch.get_msa(msa, status);
        if (msa.size() != in_batch.size()) throw std::runtime_error("MSA count does not match the windows of the batch");
    }
    else
    {
        batch.get_consensus(consensus, coverage, status);
        if (consensus.size() != in_batch.size()) throw std::runtime_error("consensus count does not match the windows of the batch");
    }
    for (size_t k = 0; k < in_batch.size(); k++)
    {
        const size_t w = in_batch[k];
        if (w >= n) continue;
        if (want_msa)
            out.msa[w] = std::move(msa[k]);
        else
        {
            out.consensus[w] = std::move(consensus[k]);
            out.coverage[w]  = std::move(coverage[k]);
        }
        out.status[w] = status[k];
    }
}

void rethrow_first(const std::vector<std::exception_ptr>& errors)
{
    for (const std::exception_ptr& e : errors)
        if (e) std::rethrow_exception(e);
}

// ---- workers on a shared cursor ---------------------------------------------------------------------------------------------
struct SharedCursor
{
    std::mutex mutex;
    WindowQueue queue;
};

// One worker: fills its batch from the cursor, runs it, stores by global index; until the windows run out.
// Every worker's Batch exists before any of them fills: the clock of the reference's multi-batch benchmark starts there
// (cudapoa/benchmarks/multi_batch.hpp: the batches are created in the constructor, process_batches() is what is timed).
void worker_loop(int32_t worker, int32_t device, cudaStream_t stream, DefaultDeviceAllocator allocator, int64_t memory,
                 const BatchConfig& batch_size, const MultiDeviceConfig& config, const std::vector<std::vector<std::string>>& windows,
                 SharedCursor& cursor, MultiDeviceOutput& out, std::atomic<int32_t>& launches, Rendezvous& created, ResultClock& results,
                 const WindowWeights* weights)
{
    scoped_device_switch dev(device);
    std::unique_ptr<Batch> batch = create_batch(device, stream, allocator, memory, config.output_mask, batch_size, config.gap_score,
                                                config.mismatch_score, config.match_score);
    created.arrive(static_cast<size_t>(worker));
    const bool want_msa = (config.output_mask & OutputType::msa) != 0;
    // A fill stops at a whole number of device rounds: the device runs `resident` windows side by side (one wavefront per SIMD;
    // 0 = a configuration that is not one wavefront per window), and a launch of 1400 windows lasts two rounds like one of 2048
    // -- the 376 windows of its second round would have filled the SIMDs together with another worker's. Measured
    // (profiles/r06_multibatch_timeline.txt): 2048 full-band windows over two batches of 16 GB, 1400 + 648: 145 ms; 1024 + 1024: 1xx ms.
    int32_t fill_cap = INT32_MAX;
    {
        const gwhip_poa_config dc = make_device_config(batch_size, config.output_mask, config.gap_score, config.mismatch_score, config.match_score);
        const int32_t resident    = gwhip_poa_resident_windows(&dc);
        if (const char* e = std::getenv("GW_POA_FILL_ROUNDS"); e != nullptr && e[0] == '0') {}
        else if (resident > 0) fill_cap = resident; // (a batch that holds less fills up as before)
    }
    std::vector<size_t> in_batch;
    for (;;)
    {
        batch->reset();
        in_batch.clear();
        {
            // the cursor only moves under the lock: a window is taken by exactly one worker
            std::lock_guard<std::mutex> guard(cursor.mutex);
            fill_batch(*batch, in_batch, cursor.queue, fill_cap, windows, worker, out, "a batch of this configuration cannot hold a single window", weights);
        }
        if (batch->get_total_poas() == 0)
        {
            // everything this worker took is stored: the timed region of the reference's multi-batch benchmark ends here (its
            // batches outlive process_batches(); releasing a Batch -- its pinned staging block above all -- is not part of it)
            results.stamp();
            break;
        }
        batch->generate_poa();
        launches++;
        store_results(*batch, want_msa, in_batch, out);
    }
}
// The weights of a weighted call against its windows: one entry per window and per read, a read's weights empty or as many
// as its bases, none of them negative -- anything else throws before a worker starts. A window one of whose reads carries
// nothing but zeros is refused as a whole, with the status a Batch gives that read, and never reaches a batch.
void check_weights(const std::vector<std::vector<std::string>>& windows, const WindowWeights& weights, MultiDeviceOutput& out)
{
    if (weights.size() != windows.size()) throw std::invalid_argument("weights: one entry per window is needed");
    for (size_t w = 0; w < windows.size(); w++)
    {
        if (weights[w].size() != windows[w].size()) throw std::invalid_argument("weights: window " + std::to_string(w) + " needs one entry per read");
        for (size_t r = 0; r < windows[w].size(); r++)
        {
            const std::vector<int8_t>& of_read = weights[w][r];
            if (of_read.empty()) continue;
            if (of_read.size() != windows[w][r].size())
                throw std::invalid_argument("weights: read " + std::to_string(r) + " of window " + std::to_string(w) + " needs one weight per base");
            bool all_zero = true;
            for (int8_t x : of_read)
            {
                throw_on_negative(x, "Base weights need to be non-negative");
                if (x > 0) all_zero = false;
            }
            if (all_zero) out.status[w] = StatusType::zero_weighted_poa_sequence;
        }
    }
}

void run_multi_device(MultiDeviceOutput& out, const std::vector<std::vector<std::string>>& windows, const WindowWeights* weights,
                      const BatchConfig& batch_size, const MultiDeviceConfig& config);
} // namespace

void process_windows_multi_device(MultiDeviceOutput& out, const std::vector<std::vector<std::string>>& windows,
                                  const BatchConfig& batch_size, const MultiDeviceConfig& config)
{
    run_multi_device(out, windows, nullptr, batch_size, config);
}

void process_windows_multi_device(MultiDeviceOutput& out, const std::vector<std::vector<std::string>>& windows,
                                  const std::vector<std::vector<std::vector<int8_t>>>& weights, const BatchConfig& batch_size,
                                  const MultiDeviceConfig& config)
{
    run_multi_device(out, windows, &weights, batch_size, config);
}

namespace
{
void run_multi_device(MultiDeviceOutput& out, const std::vector<std::vector<std::string>>& windows, const WindowWeights* weights,
                      const BatchConfig& batch_size, const MultiDeviceConfig& config)
{
    if (config.devices.empty()) throw std::invalid_argument("at least one device is needed");
    if (config.batches_per_device < 1) throw std::invalid_argument("batches_per_device has to be at least 1");
    int32_t n_devices = 0;
    GW_CU_CHECK_ERR(hipGetDeviceCount(&n_devices));
    std::map<int32_t, int32_t> entries_of_device;
    for (int32_t d : config.devices)
    {
        if (d < 0 || d >= n_devices) throw std::invalid_argument("device id out of range: " + std::to_string(d));
        entries_of_device[d]++;
    }
    prepare_output(out, windows.size(), (config.output_mask & OutputType::msa) != 0);
    if (weights != nullptr) check_weights(windows, *weights, out);
    if (windows.empty()) return;

    // one allocator per entry of `devices`, shared by that entry's batches (as multi_batch.hpp:52-60 shares one)
    struct Group
    {
        int32_t device;
        int64_t memory;
        DefaultDeviceAllocator allocator;
    };
    std::vector<Group> groups;
    for (int32_t d : config.devices)
    {
        scoped_device_switch dev(d);
        int64_t memory = config.memory_per_device;
        if (memory < 0)
        {
            size_t free_bytes = 0, total_bytes = 0;
            GW_CU_CHECK_ERR(hipMemGetInfo(&free_bytes, &total_bytes));
            // free memory is read before any group of this device allocates: the entries naming the device share it
            memory = static_cast<int64_t>(config.memory_fraction * static_cast<double>(free_bytes)) / entries_of_device[d];
        }
        groups.push_back(Group{d, memory, DefaultDeviceAllocator()});
    }
    // allocate after all the free-memory readings
    for (Group& g : groups)
    {
        scoped_device_switch dev(g.device);
        g.allocator = DefaultDeviceAllocator(static_cast<size_t>(g.memory), nullptr);
    }

    SharedCursor cursor;
    cursor.queue.size = windows.size();
    std::atomic<int32_t> launches{0};
    ResultClock results;
    results.begin = Clock::now();
    // every stream exists before the first worker starts (a failing hipStreamCreate must not leave joinable threads behind)
    OwnedStreams streams;
    for (Group& g : groups)
        for (int32_t b = 0; b < config.batches_per_device; b++) streams.create(g.device);
    const size_t workers = groups.size() * static_cast<size_t>(config.batches_per_device);
    std::vector<std::exception_ptr> errors(workers);
    std::vector<std::thread> threads;
    std::atomic<bool> abandoned{false};
    Rendezvous created(workers, workers, abandoned);
    threads.reserve(workers);
    {
        JoinAll join{threads};
        int32_t worker = 0;
        try
        {
            for (Group& g : groups)
                for (int32_t b = 0; b < config.batches_per_device; b++, worker++)
                {
                    cudaStream_t stream  = streams.items[static_cast<size_t>(worker)].second;
                    const int64_t memory = g.memory / config.batches_per_device;
                    threads.emplace_back([&, worker, stream, memory, device = g.device, allocator = g.allocator]() {
                        try
                        {
                            worker_loop(worker, device, stream, allocator, memory, batch_size, config, windows, cursor, out, launches, created, results, weights);
                        }
                        catch (...)
                        {
                            errors[static_cast<size_t>(worker)] = std::current_exception();
                            created.arrive(static_cast<size_t>(worker)); // a failed creation releases the others
                        }
                    });
                }
        }
        catch (...)
        {
            abandoned.store(true); // std::thread could not start a worker: the started ones must not wait for it
            throw;
        }
    }
    const auto t_end = Clock::now();
    out.seconds      = std::chrono::duration<double>(t_end - results.begin).count();
    if (created.complete())
        out.seconds_after_creation =
            std::chrono::duration<double>((results.last() > created.all_arrived ? results.last() : t_end) - created.all_arrived).count();
    out.launches = launches.load();
    rethrow_first(errors);
}
} // namespace

// ---- size classes -------------------------------------------------------------------------------------------------------
void plan_size_classes(SizeClassPlan& plan, const std::vector<int32_t>& longest, const std::vector<int32_t>& reads, bool msa_flag,
                       int32_t band_width, BandMode band_mode, float adaptive_storage_factor, float graph_length_factor,
                       int32_t max_pred_distance, int32_t mismatch_score, int32_t gap_score, int32_t match_score)
{
    if (longest.size() != reads.size()) throw std::invalid_argument("one read count per window");
    plan = SizeClassPlan{};
    int32_t top = 0;
    for (int32_t l : longest) top = std::max(top, l);
    if (top <= 0) return;
    // class k: longest read in (top / 2^(k+1), top / 2^k]; everything below top / 64 shares the last class
    constexpr int kClasses = 6;
    std::vector<std::vector<int32_t>> members(kClasses);
    for (size_t w = 0; w < longest.size(); ++w)
    {
        int k = 0;
        while (k + 1 < kClasses && static_cast<int64_t>(longest[w]) * (int64_t(2) << k) <= top) ++k;
        members[static_cast<size_t>(k)].push_back(static_cast<int32_t>(w));
    }
    for (const std::vector<int32_t>& m : members)
    {
        if (m.empty()) continue;
        int32_t len = 0, most = 0;
        for (int32_t w : m)
        {
            len  = std::max(len, longest[static_cast<size_t>(w)]);
            most = std::max(most, reads[static_cast<size_t>(w)]);
        }
        // a band cannot be wider than the reads it is laid over (batch.cu:96-97): short classes keep the requested width only if they can
        const BatchConfig cfg(std::max(len, band_width), most, band_width, band_mode, adaptive_storage_factor, graph_length_factor, max_pred_distance);
        const gwhip_poa_config dc = make_device_config(cfg, static_cast<int8_t>(msa_flag ? OutputType::msa : OutputType::consensus), gap_score,
                                                       mismatch_score, match_score);
        int64_t per_poa = 0, per_matrix = 0;
        gwhip_poa_bytes_per_window(&dc, &per_poa, &per_matrix);
        plan.configs.push_back(cfg);
        plan.groups.push_back(m);
        plan.bytes_per_window.push_back(per_poa + per_matrix);
        plan.total_bytes += static_cast<int64_t>(m.size()) * (per_poa + per_matrix);
    }
}

std::vector<int32_t> size_class_admission_gates(const SizeClassPlan& plan, int32_t compute_units)
{
    const size_t classes = plan.groups.size();
    std::vector<int32_t> gate_on(classes, -1);
    const int64_t cus  = compute_units > 0 ? compute_units : 256;
    const int64_t room = cus + cus / 4;
    int64_t in_group   = 0;
    int32_t prev_last = -1, last = -1;
    for (size_t k = 0; k < classes; ++k)
    {
        if (plan.groups[k].empty()) continue;
        const int64_t w = static_cast<int64_t>(plan.groups[k].size());
        if (last >= 0 && in_group + w > room)
        {
            prev_last = last;
            in_group  = 0;
        }
        gate_on[k] = prev_last;
        in_group += w;
        last = static_cast<int32_t>(k);
    }
    return gate_on;
}


namespace
{
// One call of process_windows_size_classes: what its class workers share. A worker is one host thread with the stream,
// the memory share and the Batch of its class.
struct SizeClassRun
{
    const std::vector<std::vector<std::string>>& windows;
    const SizeClassPlan& plan;
    MultiDeviceOutput& out;
    const int32_t device;
    const int8_t output_mask;
    const int16_t gap_score, mismatch_score, match_score;
    const bool want_msa;
    const bool trace; // GW_SIZE_CLASS_TRACE (debugging): host-side timeline on stderr
    const size_t classes, active_classes;

    std::vector<int64_t> share; // device bytes of each class
    // The classes' first launches are submitted in plan order (longest reads first) and on streams whose priority falls in
    // the same order: a window is one chain of dependent steps on one CU, the set lasts at least as long as its heaviest
    // window, so that window's class must own its CUs from the first moment instead of queueing behind hundreds of light
    // blocks that happened to be submitted a millisecond earlier.
    std::vector<int32_t> launch_rank;
    std::atomic<int32_t> launch_turn{0};
    // Admission by residency: a window occupies a CU for its whole life, so the device holds about one window per CU at
    // a time. Classes are admitted in plan order while their windows (a quarter more than there are CUs: the first to
    // finish make room at once) fit; the next group of classes is gated, on the device, on the end of the lightest class
    // of the group before it. Admitting everything at once only makes the long chains of the heavy classes queue for CUs
    // behind light windows -- and those chains are what the set waits for at the end.
    std::vector<int32_t> gate_on;
    OwnedEvents class_done; // [class], recorded behind every launch of the class
    OwnedStreams class_streams;
    std::vector<cudaStream_t> stream_of;

    std::atomic<bool> abandoned{false}; // a worker thread could not be started: nobody waits for it
    // every class's Batch exists (or its creation failed): the fill-inclusive clock (the reference's multi-batch region,
    // cudapoa/benchmarks/multi_batch.hpp:72-177, creates all batches first and times all of the filling) starts, and no
    // class fills before that point -- a class that was created early would otherwise do its filling outside the clock
    Rendezvous created;
    // every class's first fill is done (or the class failed): the compute clock starts
    Rendezvous filled;
    std::atomic<int32_t> batches_created{0}, launches{0};
    // the clocks stop when the last results have been handed over: releasing the slabs (hundreds of GB for a long-read set,
    // most of a second) is not part of generate_poa() + get_msa()
    ResultClock results;
    std::vector<std::exception_ptr> errors;

    SizeClassRun(MultiDeviceOutput& out_, const std::vector<std::vector<std::string>>& windows_, const SizeClassPlan& plan_, size_t active, int32_t device_,
                 int64_t memory_budget, int8_t mask, int16_t gap, int16_t mismatch, int16_t match)
        : windows(windows_), plan(plan_), out(out_), device(device_), output_mask(mask), gap_score(gap), mismatch_score(mismatch), match_score(match)
        , want_msa((mask & OutputType::msa) != 0), trace(std::getenv("GW_SIZE_CLASS_TRACE") != nullptr), classes(plan_.configs.size())
        , active_classes(active), share(classes), launch_rank(classes, 0), stream_of(classes, nullptr), created(classes, active, abandoned)
        , filled(classes, active, abandoned), errors(classes)
    {
        // every class gets its planned bytes (+ slack for alignment and one spare window), scaled down when the plan exceeds the budget
        const int64_t slack_total = static_cast<int64_t>(classes) * (int64_t(64) << 20);
        auto planned              = [&](size_t k) { return (static_cast<int64_t>(plan.groups[k].size()) + 1) * plan.bytes_per_window[k]; };
        int64_t want              = slack_total;
        for (size_t k = 0; k < classes; ++k) want += planned(k);
        const double scale = want > memory_budget ? static_cast<double>(memory_budget - slack_total) / static_cast<double>(want - slack_total) : 1.0;
        for (size_t k = 0; k < classes; ++k)
            share[k] = std::max<int64_t>(2 * plan.bytes_per_window[k], static_cast<int64_t>(scale * static_cast<double>(planned(k)))) + (int64_t(64) << 20);
        int32_t rank = 0;
        for (size_t k = 0; k < classes; ++k)
            if (!plan.groups[k].empty()) launch_rank[k] = rank++;
        int priority_least = 0, priority_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&priority_least, &priority_greatest);
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        gate_on = size_class_admission_gates(plan, cus);
        // events and streams of the class workers are created up front: released on every exit path
        for (size_t k = 0; k < classes; ++k) class_done.create();
        for (size_t k = 0; k < classes; ++k)
            if (!plan.groups[k].empty())
                // numerically lower = more urgent; the range is narrow (three levels on this hardware), later classes share the last
                stream_of[k] = class_streams.create(device, true, std::min(priority_least, priority_greatest + launch_rank[k]));
    }

    double since_begin_ms() const { return std::chrono::duration<double, std::milli>(Clock::now() - results.begin).count(); }
    void wait_for_turn(size_t k) const
    {
        while (launch_turn.load() < launch_rank[k] && !abandoned.load()) std::this_thread::yield();
    }

    // heaviest windows first: blocks are dispatched in window order, and a class that does not fit the free CUs at once
    // should not keep its long chains for the end
    std::vector<int32_t> heaviest_first(size_t k) const
    {
        std::vector<std::pair<int64_t, int32_t>> keyed;
        keyed.reserve(plan.groups[k].size());
        for (int32_t w : plan.groups[k])
        {
            int64_t bases = 0;
            for (const std::string& read : windows[static_cast<size_t>(w)]) bases += static_cast<int64_t>(read.size());
            keyed.emplace_back(-bases, w);
        }
        std::stable_sort(keyed.begin(), keyed.end());
        std::vector<int32_t> order;
        for (const auto& kw : keyed) order.push_back(kw.second);
        return order;
    }

    void work(size_t k)
    {
        scoped_device_switch d(device);
        cudaStream_t stream = stream_of[k];
        DefaultDeviceAllocator allocator(static_cast<size_t>(share[k]), stream);
        std::unique_ptr<Batch> batch =
            create_batch(device, stream, allocator, share[k], output_mask, plan.configs[k], gap_score, mismatch_score, match_score);
        batches_created.fetch_add(1);
        created.arrive(k);
        const std::vector<int32_t> order = heaviest_first(k);
        WindowQueue queue{&order, order.size(), 0};
        bool first_launch = true;
        std::vector<size_t> in_batch;
        while (!queue.empty())
        {
            batch->reset();
            in_batch.clear();
            fill_batch(*batch, in_batch, queue, INT32_MAX, windows, static_cast<int32_t>(k), out, "a batch of this size class cannot hold a single window");
            filled.arrive(k);
            if (first_launch) // submission order of the classes' first launches
            {
                wait_for_turn(k);
                // (the gate's event was recorded before its class passed the turn on)
                if (gate_on[k] >= 0) GW_CU_CHECK_ERR(hipStreamWaitEvent(stream, class_done.items[static_cast<size_t>(gate_on[k])], 0));
            }
            if (trace) std::fprintf(stderr, "[size classes] class %zu: generate_poa() called at %.1f ms\n", k, since_begin_ms());
            if (batch->get_total_poas() > 0) batch->generate_poa();
            if (trace) std::fprintf(stderr, "[size classes] class %zu: generate_poa() returned at %.1f ms\n", k, since_begin_ms());
            // the gate of later class groups: (re-)recorded behind EVERY launch of this class, so a waiter that
            // arrives late waits for the class's last submitted launch, not only for its first
            GW_CU_CHECK_ERR(hipEventRecord(class_done.items[k], stream));
            if (first_launch)
            {
                first_launch = false;
                launch_turn.fetch_add(1);
            }
            if (batch->get_total_poas() == 0) continue;
            launches++;
            if (trace && want_msa)
            {
                GW_CU_CHECK_ERR(hipStreamSynchronize(stream));
                std::fprintf(stderr, "[size classes] class %zu: kernels done at %.1f ms\n", k, since_begin_ms());
            }
            store_results(*batch, want_msa, in_batch, out);
            if (trace && want_msa) std::fprintf(stderr, "[size classes] class %zu: get_msa() returned at %.1f ms\n", k, since_begin_ms());
            results.stamp();
        }
        filled.arrive(k);
    }

    void run_class(size_t k)
    {
        try
        {
            work(k);
        }
        catch (...)
        {
            errors[k] = std::current_exception();
            created.arrive(k); // the error path releases both rendezvous too
            filled.arrive(k);
            // a class that failed before its first launch still passes the turn on
            wait_for_turn(k);
            int32_t mine_turn = launch_rank[k];
            launch_turn.compare_exchange_strong(mine_turn, launch_rank[k] + 1);
        }
    }
};
} // namespace

void process_windows_size_classes(MultiDeviceOutput& out, const std::vector<std::vector<std::string>>& windows,
                                  const SizeClassPlan& plan, int32_t device, int64_t memory_budget, int8_t output_mask,
                                  int16_t gap_score, int16_t mismatch_score, int16_t match_score, double* compute_seconds)
{
    prepare_output(out, windows.size(), (output_mask & OutputType::msa) != 0);
    if (compute_seconds) *compute_seconds = 0;
    const size_t classes = plan.configs.size();
    if (windows.empty() || classes == 0) return;
    scoped_device_switch dev(device);
    size_t active_classes = 0;
    for (size_t k = 0; k < classes; ++k) active_classes += plan.groups[k].empty() ? 0 : 1;
    if (active_classes == 0) return;
    SizeClassRun run(out, windows, plan, active_classes, device, memory_budget, output_mask, gap_score, mismatch_score, match_score);
    std::vector<std::thread> threads;
    JoinAll join_on_exit{threads};
    run.results.begin = Clock::now();
    threads.reserve(classes);
    try
    {
        for (size_t k = 0; k < classes; ++k)
            if (!plan.groups[k].empty()) threads.emplace_back([&run, k]() { run.run_class(k); });
    }
    catch (...)
    {
        // std::thread could not start a worker (std::system_error): the started ones must not spin at the barriers for it;
        // JoinAll joins them on the way out and the error surfaces
        run.abandoned.store(true);
        throw;
    }
    for (std::thread& t : threads) t.join();
    const auto t_end = Clock::now();
    out.seconds      = std::chrono::duration<double>(t_end - run.results.begin).count();
    if (compute_seconds) *compute_seconds = std::chrono::duration<double>((run.results.stamped() ? run.results.last() : t_end) - run.filled.all_arrived).count();
    out.launches = run.launches.load();
    if (run.batches_created.load() == static_cast<int32_t>(active_classes) && run.results.stamped())
        out.seconds_after_creation = std::chrono::duration<double>(run.results.last() - run.created.all_arrived).count();
    rethrow_first(run.errors);
}

} // namespace cudapoa
} // namespace genomeworks
} // namespace claraparabricks
