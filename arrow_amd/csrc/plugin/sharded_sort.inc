// array_sort_indices over a row-sharded uint64 / int64 array, RCCL called directly (no torch).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- multi-GPU sort, RCCL called directly
// SURVEY.md 8(e).  The reference sorts a chunked array chunk by chunk and merges (ChunkedArraySorter,
// kernels/vector_sort.cc); with one row shard per GPU the merge becomes a range partition in front of the local sorts:
//   0. the window [min, max] of the order-transformed keys of all shards (arx_sort_key_range + one all-gather of
//      16 bytes per rank): ids and timestamps share their top bits, splitter bins are taken inside the window;
//   1. a histogram of 2^bits bins of the window per shard (arx_sort_key_histogram_window), all-gathered with the shard
//      lengths -> world - 1 splitters at equal shares of the valid rows, and every rank's slice of the result;
//   2. the shard's rows partitioned by destination rank as 12-byte {key, local row} records, its null rows (row numbers
//      only) in the block of the last (nulls at the end) / first rank (arx_sort_partition_records_window);
//   3. the block sizes (one all-gather) and ONE exchange: an ncclSend / ncclRecv pair per peer inside one group;
//   4. records -> keys + GLOBAL row numbers in source order (arx_sort_unpack_records: equal keys stay in global row
//      order), the local stable sort (arx_sort_indices_64) and one gather of the global rows (arx_take).
// The result of rank r is the slice [start, start + length) of ArraySortIndices' permutation of the concatenated
// shards (vector_array_sort.cc:524-540; null placement vector_sort_internal.h:225-293).  The same data path as
// arrow_amd/parallel.py sharded_sort_indices; every reduction is an all-gather + a host fold (three small ones), so the
// RCCL surface stays the group-by's: ncclAllGather, ncclSend / ncclRecv, ncclGroupStart / End.
Status ShardedSortIndices(const ShardedComm& c, const ArrayData& values, bool descending, bool nulls_first, int splitter_bits,
                          std::shared_ptr<ArrayData>* out_indices, int64_t* out_start, double* stage_ms) {
  const bool is_signed = values.type->id() == Type::INT64;
  if (!is_signed && values.type->id() != Type::UINT64) {
    return Status::NotImplemented("arrow_amd sharded sort: uint64 / int64 keys");
  }
  if (!DataOnRocm(values)) return Status::Invalid("arrow_amd sharded sort: device-resident shards");
  if (splitter_bits < 1 || splitter_bits > 12) return Status::Invalid("arrow_amd sharded sort: 1..12 splitter bits");
  ARROW_ASSIGN_OR_RAISE(const RcclApi* api, Rccl());
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  StageClock clock(st, stage_ms);
  const int world = c.world, rank = c.rank;
  const int64_t n = values.length;
  const int order = descending ? ARX_SORT_DESCENDING : ARX_SORT_ASCENDING;
  const int placement = nulls_first ? ARX_NULLS_AT_START : ARX_NULLS_AT_END;
  const int target = nulls_first ? 0 : world - 1;   // the rank that takes every shard's null rows
  ArxSpan dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(values), &dv));
  auto dev_ptr = [](const std::shared_ptr<Buffer>& b) { return reinterpret_cast<void*>(b->mutable_address()); };
  // all-gather of `count` int64 per rank, folded on the host
  auto gather_i64 = [&](const std::shared_ptr<Buffer>& mine, int64_t count, std::vector<int64_t>* all) -> Status {
    ARROW_ASSIGN_OR_RAISE(auto everybody, AllocDevice(count * world * 8));
    RCCL_RETURN_NOT_OK(api, api->AllGather(dev_ptr(mine), dev_ptr(everybody), static_cast<size_t>(count), kNcclInt64, c.comm, st));
    all->resize(static_cast<size_t>(count) * world);
    HIP_RETURN_NOT_OK(hipMemcpyAsync(all->data(), dev_ptr(everybody), all->size() * 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    return Status::OK();
  };

  // ---- 0. the key window.  The same gather carries what decides the SAMPLED form (round 6, as arrow_amd/parallel.py): "this
  //         shard may have nulls" and the shard's length — no shard with nulls and world x the longest shard < 2^32 rows means
  //         the records form below is certain and nothing needs exact per-bin counts: the range and the histogram come from
  //         one tile of 8192 rows in 2^shift (a key outside the sampled, widened window falls into its first / last bin).
  const bool may_have_nulls = values.buffers[0] != nullptr;   // (a device array's null count is not to be trusted)
  const int sample_knob = g_sharded_sort_sample_shift.load();
  const int64_t sample_min_rows = g_sharded_sort_sample_min_rows.load();
  const bool records_allowed = g_sharded_sort_records.load();
  const int my_shift = (records_allowed && sample_knob > 0 && !may_have_nulls && n >= sample_min_rows) ? sample_knob : 0;
  ARROW_ASSIGN_OR_RAISE(auto d_range, AllocDevice(32));
  HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(d_range), 0, 32, st));
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_key_range_sampled(&dv, is_signed ? 1 : 0, order, my_shift, static_cast<uint64_t*>(dev_ptr(d_range)), st)));
  const int64_t extra[2] = {(may_have_nulls || !records_allowed) ? 1 : 0, n};
  HIP_RETURN_NOT_OK(hipMemcpyAsync(static_cast<int64_t*>(dev_ptr(d_range)) + 2, extra, 16, hipMemcpyHostToDevice, st));
  std::vector<int64_t> ranges;
  ARROW_RETURN_NOT_OK(gather_i64(d_range, 4, &ranges));
  uint64_t inv_min = 0, key_max = 0;   // {max of ~key, max of key} over every shard's valid rows
  int64_t any_nulls = 0, longest = 0;
  for (int r = 0; r < world; ++r) {
    inv_min = std::max(inv_min, static_cast<uint64_t>(ranges[4 * r]));
    key_max = std::max(key_max, static_cast<uint64_t>(ranges[4 * r + 1]));
    any_nulls = std::max(any_nulls, ranges[4 * r + 2]);
    longest = std::max(longest, ranges[4 * r + 3]);
  }
  const bool sampled = sample_knob > 0 && any_nulls == 0 && longest * world < (int64_t(1) << 32) && longest >= sample_min_rows;
  uint64_t key_min = ~inv_min;
  if (sampled && key_max > key_min) {   // a sample misses a few keys at both ends
    const uint64_t margin = ((key_max - key_min) >> 6) + 1;
    key_min = key_min > margin ? key_min - margin : 0;
    key_max = key_max < ~uint64_t(0) - margin ? key_max + margin : ~uint64_t(0);
  }
  ArxSortKeyWindow window{0, 0, 0};
  if (key_max > key_min) {   // (no valid row anywhere: min = 2^64 - 1 > max = 0; one distinct key: nothing to split)
    window.key_min = key_min;
    window.shift = __builtin_clzll(key_max - key_min);
  }

  // ---- 1. histogram of the window's bins + the shard length, everybody's
  const int nbins = 1 << splitter_bits;
  ARROW_ASSIGN_OR_RAISE(auto d_stats, AllocDevice((nbins + 1) * 8));
  HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(d_stats), 0, static_cast<size_t>(nbins + 1) * 8, st));
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_key_histogram_window_sampled(&dv, is_signed ? 1 : 0, order, splitter_bits, &window, sampled ? sample_knob : 0,
                                                                    static_cast<uint64_t*>(dev_ptr(d_stats)), st)));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(static_cast<int64_t*>(dev_ptr(d_stats)) + nbins, &n, 8, hipMemcpyHostToDevice, st));
  std::vector<int64_t> stats;
  ARROW_RETURN_NOT_OK(gather_i64(d_stats, nbins + 1, &stats));
  ARROW_RETURN_NOT_OK(clock.Mark());   // histogram
  std::vector<int64_t> cum(nbins, 0), lens(world), valid(world, 0), offsets(world, 0);
  for (int r = 0; r < world; ++r) {
    const int64_t* s = stats.data() + static_cast<size_t>(r) * (nbins + 1);
    for (int b = 0; b < nbins; ++b) {
      cum[b] += s[b];
      valid[r] += s[b];
    }
    lens[r] = s[nbins];
    if (sampled) valid[r] = lens[r];   // (no shard has nulls; the histogram holds the rows of the SAMPLE)
  }
  for (int b = 1; b < nbins; ++b) cum[b] += cum[b - 1];
  for (int r = 1; r < world; ++r) offsets[r] = offsets[r - 1] + lens[r - 1];
  const int64_t total_valid = cum[nbins - 1];   // (sampled: of the sample — the splitters are its quantiles)
  int64_t total_rows = 0;
  for (int r = 0; r < world; ++r) total_rows += lens[r];
  const int64_t total_nulls = sampled ? 0 : total_rows - total_valid;
  std::vector<uint32_t> split(std::max(world - 1, 1), static_cast<uint32_t>(nbins));
  for (int p = 1; p < world; ++p) {
    const int64_t want = (total_valid * p + world - 1) / world;
    int64_t b = nbins;
    if (total_valid > 0) b = (std::lower_bound(cum.begin(), cum.end(), want) - cum.begin()) + 1;
    split[p - 1] = static_cast<uint32_t>(std::min<int64_t>(b, nbins));
  }
  // what every rank will own (known without another collective): the bins below its splitter
  std::vector<int64_t> edges(world + 1, 0), owned(world, 0);
  for (int p = 1; p < world; ++p) edges[p] = split[p - 1];
  edges[world] = nbins;
  for (int r = 0; r < world; ++r) {
    if (edges[r + 1] > edges[r]) owned[r] = cum[edges[r + 1] - 1] - (edges[r] > 0 ? cum[edges[r] - 1] : 0);
    if (r == target) owned[r] += total_nulls;
  }
  int64_t start = 0;
  for (int r = 0; r < rank; ++r) start += owned[r];

  // ---- Round 6: no nulls anywhere and global rows that fit 32 bits — the records carry GLOBAL rows, the partition needs no
  //      stable pass (arx_sort_partition_records_global) and the receiver sorts what it got by (key, row) where it lies
  //      (arx_sort_records): no unpack, no column sort, no gather.  What every rank owns comes from the gathered counts.
  if (records_allowed && total_nulls == 0 && total_rows < (int64_t(1) << 32)) {
    ARROW_ASSIGN_OR_RAISE(auto records, AllocDevice(std::max<int64_t>(n, 1) * 12));
    ARROW_ASSIGN_OR_RAISE(auto d_counts, AllocDevice(world * 8));
    HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(d_counts), 0, static_cast<size_t>(world) * 8, st));
    ARROW_ASSIGN_OR_RAISE(auto pws, AllocDevice(1024));
    ARROW_RETURN_NOT_OK(FromArx(arx_sort_partition_records_global(&dv, is_signed ? 1 : 0, order, splitter_bits, &window, split.data(), world,
                                                                  static_cast<uint32_t>(offsets[rank]), dev_ptr(pws), 1024,
                                                                  static_cast<ArxSortRecord*>(dev_ptr(records)),
                                                                  static_cast<int64_t*>(dev_ptr(d_counts)), st)));
    ARROW_RETURN_NOT_OK(clock.Mark());   // partition
    std::vector<int64_t> all_counts;
    ARROW_RETURN_NOT_OK(gather_i64(d_counts, world, &all_counts));
    std::vector<int64_t> soff(world + 1, 0), roff(world + 1, 0), mine(world, 0);
    for (int p = 0; p < world; ++p) {
      soff[p + 1] = soff[p] + all_counts[static_cast<size_t>(rank) * world + p];
      roff[p + 1] = roff[p] + all_counts[static_cast<size_t>(p) * world + rank];
      for (int src = 0; src < world; ++src) mine[p] += all_counts[static_cast<size_t>(src) * world + p];
    }
    int64_t my_start = 0;
    for (int r = 0; r < rank; ++r) my_start += mine[r];
    const int64_t m = roff[world];
    if (m != mine[rank] || soff[world] != n) {
      return Status::Invalid("arrow_amd sharded sort: rank ", rank, " counts disagree (", m, " received, ", mine[rank], " owned, ", soff[world],
                             " sent of ", n, " rows)");
    }
    ARROW_ASSIGN_OR_RAISE(auto inbox, AllocDevice(std::max<int64_t>(m, 1) * 12));
    RCCL_RETURN_NOT_OK(api, api->GroupStart());
    int group_rc = 0;
    for (int p = 0; p < world && group_rc == 0; ++p) {
      if (soff[p + 1] > soff[p]) {
        group_rc = api->Send(static_cast<const uint8_t*>(dev_ptr(records)) + soff[p] * 12, static_cast<size_t>(soff[p + 1] - soff[p]) * 12,
                             kNcclUint8, p, c.comm, st);
      }
      if (group_rc == 0 && roff[p + 1] > roff[p]) {
        group_rc = api->Recv(static_cast<uint8_t*>(dev_ptr(inbox)) + roff[p] * 12, static_cast<size_t>(roff[p + 1] - roff[p]) * 12, kNcclUint8,
                             p, c.comm, st);
      }
    }
    const int end_rc = api->GroupEnd();   // (closed whatever happened: the peers would block in theirs)
    RCCL_RETURN_NOT_OK(api, group_rc);
    RCCL_RETURN_NOT_OK(api, end_rc);
    ARROW_RETURN_NOT_OK(clock.Mark());   // exchange
    ARROW_ASSIGN_OR_RAISE(auto result, AllocDevice(std::max<int64_t>(m, 1) * 8));
    if (m > 0) {
      const size_t sort_ws_bytes = arx_sort_indices_workspace_bytes(m);
      ARROW_ASSIGN_OR_RAISE(auto sort_ws_buf, AllocAligned(static_cast<int64_t>(sort_ws_bytes)));
      void* sort_ws = sort_ws_buf.ptr;
      ARROW_RETURN_NOT_OK(FromArx(arx_sort_records(static_cast<const ArxSortRecord*>(dev_ptr(inbox)), m, sort_ws, sort_ws_bytes,
                                                   static_cast<uint64_t*>(dev_ptr(result)), st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    ARROW_RETURN_NOT_OK(clock.Mark());   // local sort
    *out_indices = ArrayData::Make(arrow::uint64(), m, {nullptr, std::move(result)}, 0);
    *out_start = my_start;
    g_sharded_sort_records_runs.fetch_add(1);
    CountGpu(kFnSort);
    return Status::OK();
  }

  // ---- 2. stable partition by destination, packed records (+ this shard's null rows)
  const size_t ws_bytes = arx_sort_indices_workspace_bytes(std::max<int64_t>(n, 1));
  ARROW_ASSIGN_OR_RAISE(auto ws_buf, AllocAligned(static_cast<int64_t>(ws_bytes)));
  void* ws = ws_buf.ptr;
  ARROW_ASSIGN_OR_RAISE(auto records, AllocDevice(std::max<int64_t>(n, 1) * 12));
  ARROW_ASSIGN_OR_RAISE(auto d_counts, AllocDevice(world * 8));
  HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(d_counts), 0, static_cast<size_t>(world) * 8, st));
  int64_t n_valid = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_partition_records_window(&dv, is_signed ? 1 : 0, order, placement, splitter_bits, &window,
                                                                split.data(), world, ws, ws_bytes,
                                                                static_cast<ArxSortRecord*>(dev_ptr(records)),
                                                                static_cast<int64_t*>(dev_ptr(d_counts)), &n_valid, st)));
  const int64_t n_null = n - n_valid;
  ARROW_RETURN_NOT_OK(clock.Mark());   // partition

  // ---- 3. block sizes, then the ONE data exchange
  std::vector<int64_t> all_counts;
  ARROW_RETURN_NOT_OK(gather_i64(d_counts, world, &all_counts));
  std::vector<int64_t> send(world), recv_valid(world), recv_nulls(world, 0), recv(world), soff(world + 1, 0), roff(world + 1, 0);
  int64_t m_valid = 0, m_null = 0;
  for (int p = 0; p < world; ++p) {
    send[p] = all_counts[static_cast<size_t>(rank) * world + p] + (p == target ? n_null : 0);
    recv_valid[p] = all_counts[static_cast<size_t>(p) * world + rank];
    if (rank == target) recv_nulls[p] = lens[p] - valid[p];
    recv[p] = recv_valid[p] + recv_nulls[p];
    soff[p + 1] = soff[p] + send[p];
    roff[p + 1] = roff[p] + recv[p];
    m_valid += recv_valid[p];
    m_null += recv_nulls[p];
  }
  ARROW_ASSIGN_OR_RAISE(auto inbox, AllocDevice(std::max<int64_t>(roff[world], 1) * 12));
  // (a failing send / recv must not leave the group open — the peers would block in their GroupEnd: remember the first
  //  error, close the group whatever happened, then report; ADVICE r3)
  RCCL_RETURN_NOT_OK(api, api->GroupStart());
  int group_rc = 0;
  for (int p = 0; p < world && group_rc == 0; ++p) {
    if (send[p] > 0) {
      group_rc = api->Send(static_cast<const uint8_t*>(dev_ptr(records)) + soff[p] * 12,
                                        static_cast<size_t>(send[p]) * 12, kNcclUint8, p, c.comm, st);
    }
    if (group_rc == 0 && recv[p] > 0) {
      group_rc = api->Recv(static_cast<uint8_t*>(dev_ptr(inbox)) + roff[p] * 12,
                                        static_cast<size_t>(recv[p]) * 12, kNcclUint8, p, c.comm, st);
    }
  }
  const int end_rc = api->GroupEnd();
  RCCL_RETURN_NOT_OK(api, group_rc);
  RCCL_RETURN_NOT_OK(api, end_rc);
  ARROW_RETURN_NOT_OK(clock.Mark());   // exchange

  // ---- 4. unpack (keys + GLOBAL rows, compacted in source order), local stable sort, one gather
  std::vector<int64_t> meta(static_cast<size_t>(world) * 3);
  for (int s = 0; s < world; ++s) {
    meta[3 * s] = recv_valid[s];
    meta[3 * s + 1] = recv_nulls[s];
    meta[3 * s + 2] = offsets[s];
  }
  ARROW_ASSIGN_OR_RAISE(auto d_meta, AllocDevice(static_cast<int64_t>(meta.size()) * 8));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(dev_ptr(d_meta), meta.data(), meta.size() * 8, hipMemcpyHostToDevice, st));
  ARROW_ASSIGN_OR_RAISE(auto keys_recv, AllocDevice(std::max<int64_t>(m_valid, 1) * 8));
  ARROW_ASSIGN_OR_RAISE(auto rows_recv, AllocDevice(std::max<int64_t>(m_valid, 1) * 8));
  ARROW_ASSIGN_OR_RAISE(auto null_rows, AllocDevice(std::max<int64_t>(m_null, 1) * 8));
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_unpack_records(static_cast<const ArxSortRecord*>(dev_ptr(inbox)), m_valid + m_null,
                                                      static_cast<const int64_t*>(dev_ptr(d_meta)), world, nulls_first ? 1 : 0,
                                                      static_cast<uint64_t*>(dev_ptr(keys_recv)), static_cast<int64_t*>(dev_ptr(rows_recv)),
                                                      static_cast<int64_t*>(dev_ptr(null_rows)), st)));
  const int64_t m = m_valid + m_null;
  if (m != owned[rank]) {
    return Status::Invalid("arrow_amd sharded sort: rank ", rank, " received ", m, " rows, its splitters promised ", owned[rank]);
  }
  ARROW_ASSIGN_OR_RAISE(auto result, AllocDevice(std::max<int64_t>(m, 1) * 8));
  uint8_t* res = static_cast<uint8_t*>(dev_ptr(result));
  uint8_t* sorted_at = res + (nulls_first ? m_null : 0) * 8;
  if (m_valid > 0) {
    // the received keys are already order-transformed: plain ascending unsigned sort, then rows[perm]
    const size_t sort_ws_bytes = arx_sort_indices_workspace_bytes(m_valid);
    ARROW_ASSIGN_OR_RAISE(auto sort_ws_buf, AllocAligned(static_cast<int64_t>(sort_ws_bytes)));
    void* sort_ws = sort_ws_buf.ptr;
    ARROW_ASSIGN_OR_RAISE(auto perm, AllocDevice(m_valid * 8));
    const ArxSpan dkeys{nullptr, dev_ptr(keys_recv), 0, m_valid, 0};
    ARROW_RETURN_NOT_OK(FromArx(arx_sort_indices_64(&dkeys, 0, ARX_SORT_ASCENDING, ARX_NULLS_AT_END, sort_ws, sort_ws_bytes,
                                                    static_cast<uint64_t*>(dev_ptr(perm)), st)));
    const ArxSpan drows{nullptr, dev_ptr(rows_recv), 0, m_valid, 0};
    const ArxSpan dperm{nullptr, dev_ptr(perm), 0, m_valid, 0};
    ARROW_RETURN_NOT_OK(FromArx(arx_take(&drows, 8, &dperm, ARX_UINT64, sorted_at, nullptr, nullptr, st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the sort's workspace and the permutation go back to the pool)
  }
  if (m_null > 0) {
    ARROW_RETURN_NOT_OK(FromArx(arx_buffer_copy(dev_ptr(null_rows), res + (nulls_first ? 0 : m_valid) * 8, m_null * 8, st)));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  ARROW_RETURN_NOT_OK(clock.Mark());   // local sort
  *out_indices = ArrayData::Make(arrow::uint64(), m, {nullptr, std::move(result)}, 0);
  *out_start = start;
  CountGpu(kFnSort);
  return Status::OK();
}
