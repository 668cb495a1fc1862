"""CPU oracle of cudamapper's index batcher and of the cached batched driver's walk: group_into_batches and
generate_batches_of_indices as the reference's cudamapper/src/index_batcher.cu:32-138 state them, the counts refused as
its application_parameters.cpp:196-206 refuses them, and a model of the driver (include/gw_mapper_capi.h,
gw_mapper_map_batched_cached): the order of the index pairs, and how many indices are built and how many restored under
the reuse rule. Nothing here touches a GPU.

An index is (first_read, number_of_reads); a batch (query_indices, target_indices); generate_batches_of_indices returns
[(host_batch, [device_batch, ...]), ...]."""
from oracle_mapper_postprocess import group_reads_into_indices


def group_into_batches(query_indices, target_indices, query_indices_per_batch, target_indices_per_batch,
                       same_query_and_target):
    if same_query_and_target and query_indices_per_batch != target_indices_per_batch:
        raise ValueError("same_query_and_target is true, but indices_per_batch not the same")
    batches = []
    for q in range(0, len(query_indices), query_indices_per_batch):
        # the same set: only the upper triangle of the query * target matrix
        for t in range(q if same_query_and_target else 0, len(target_indices), target_indices_per_batch):
            batches.append((list(query_indices[q:q + query_indices_per_batch]),
                            list(target_indices[t:t + target_indices_per_batch])))
    return batches


def batches_of_descriptors(query_indices, target_indices, Q, q, C, c, same_query_and_target):
    if min(Q, q, C, c) < 1:
        raise ValueError("every number of indices has to be at least 1")
    if Q < q or C < c:
        raise ValueError("indices in host memory has to be larger or equal than indices in device memory")
    if same_query_and_target and Q != C:
        raise ValueError("indices_per_host_batch not the same")
    if same_query_and_target and q != c:
        raise ValueError("indices_per_device_batch not the same")
    out = []
    for host in group_into_batches(query_indices, target_indices, Q, C, same_query_and_target):
        # device batches are symmetric only where the host batch's query and target indices are the same
        same_in_batch = same_query_and_target and host[0] == host[1]
        out.append((host, group_into_batches(host[0], host[1], q, c, same_in_batch)))
    return out


def generate_batches_of_indices(query_lengths, target_lengths=None, Q=1, q=1, C=None, c=None,
                                query_basepairs_per_index=30_000_000, target_basepairs_per_index=None):
    """target_lengths None: the target set is the query set. C and c default to Q and q, the target index size to the
    query's."""
    same = target_lengths is None
    C, c = Q if C is None else C, q if c is None else c
    if target_basepairs_per_index is None:
        target_basepairs_per_index = query_basepairs_per_index
    if same and query_basepairs_per_index != target_basepairs_per_index:
        raise ValueError("basepairs_per_index not the same")
    qd = group_reads_into_indices(query_lengths, query_basepairs_per_index)
    td = qd if same else group_reads_into_indices(target_lengths, target_basepairs_per_index)
    return batches_of_descriptors(qd, td, Q, q, C, c, same)


def walk(query_indices, target_indices, all_to_all, Q=1, q=1, C=None, c=None, same_indices=None):
    """The driver's walk over already grouped indices. Returns (pairs, builds, restores): the index pairs
    ((query index), (target index)) in the order they are mapped, the number of indices built from bases and the number
    restored from a host copy.

    Per host batch every index that holds reads is visited once, queries first: taken from the device if the previous
    device batch left it there, else -- if the previous host batch left a host copy -- restored when the first device
    batch needs it, else built. What a later device batch needs gets a host copy. Then the device batches: the next
    one's indices are those it shares with the current one, the others are restored. All against all an index is
    named by its descriptor alone, otherwise by kind and descriptor. same_indices (default: all_to_all) says whether the
    batches are the upper triangle: all against all with two index sizes it is False."""
    C, c = Q if C is None else C, q if c is None else c
    same = all_to_all if same_indices is None else same_indices
    key = (lambda kind, d: (0,) + tuple(d)) if all_to_all else (lambda kind, d: (kind,) + tuple(d))

    def keys_of(batch):
        keys = []
        for kind in (0, 1):
            for d in batch[kind]:
                if d[1] > 0 and key(kind, d) not in keys:
                    keys.append(key(kind, d))
        return keys

    pairs, builds, restores = [], 0, 0
    on_device, on_host = set(), set()
    for host, device in batches_of_descriptors(query_indices, target_indices, Q, q, C, c, same):
        first = keys_of(device[0])
        later = [k for d in device[1:] for k in keys_of(d)]
        current, copies = set(), set()
        for k in keys_of(host):
            have = k in on_device
            if not have:
                if k not in on_host:
                    builds += 1
                    have = True
                elif k in first:
                    restores += 1
                    have = True
            if k in later:
                assert have or k in on_host
                copies.add(k)
            if k in first:
                assert have
                current.add(k)
        on_host = copies
        for b, batch in enumerate(device):
            following = set()
            if b + 1 < len(device):
                for k in keys_of(device[b + 1]):
                    if k not in current:
                        assert k in on_host
                        restores += 1
                    following.add(k)
            for qd in batch[0]:
                for td in batch[1]:
                    if qd[1] == 0 or td[1] == 0 or (all_to_all and td[0] < qd[0]):
                        continue
                    assert key(0, qd) in current and key(1, td) in current
                    pairs.append((tuple(qd), tuple(td)))
            if b + 1 < len(device):
                current = following
        on_device = current
    return pairs, builds, restores


def walk_reads(query_lengths, target_lengths=None, Q=1, q=1, C=None, c=None, max_basepairs_per_index=30_000_000,
               max_basepairs_per_target_index=None):
    """walk() for read sets, grouped as the driver groups them"""
    all_to_all = target_lengths is None
    t_limit = max_basepairs_per_index if max_basepairs_per_target_index is None else max_basepairs_per_target_index
    qd = group_reads_into_indices(query_lengths, max_basepairs_per_index)
    td = group_reads_into_indices(query_lengths if all_to_all else target_lengths, t_limit)
    return walk(qd, td, all_to_all, Q, q, C, c, all_to_all and t_limit == max_basepairs_per_index)


def pairs_of_map_batched(query_indices, target_indices, all_to_all):
    """the pair order of oracle_mapper_postprocess.map_batched: its two loops and its skips"""
    return [(tuple(qd), tuple(td)) for qd in query_indices for td in target_indices
            if not (qd[1] == 0 or td[1] == 0 or (all_to_all and td[0] < qd[0]))]
