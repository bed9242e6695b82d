// The sharded hash_sum group-by over RCCL, without torch: one process per GPU calls these entry points.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- multi-GPU group-by, RCCL called directly
// SURVEY.md 8(e) / GroupByNode's thread-local state -> Merge -> Finalize (acero/groupby_aggregate_node.cc:260-337) with
// ranks in place of threads.  Every rank: local aggregate of its row shard whose groups leave as 24-byte records in the
// region of the rank that owns each key, hash(key) % world (arx_groupby_sum_i64_consume_partials: no local table; shards
// with nulls and small shards: arx_groupby_sum_i64_consume into a local table + arx_groupby_export_partitioned) -> the
// per-destination counts (ncclAllGather of `world` int64 per rank) -> ONE exchange of the 24-byte records
// (ncclGroupStart + one ncclSend / ncclRecv pair per peer + ncclGroupEnd: xGMI is point to point, a pair per peer IS the
// all-to-all) -> Merge into the table of the keys this rank owns -> Finalize.  exchange = 1 is the row-level variant:
// the ROWS are partitioned and exchanged as 16-byte records (arx_groupby_partition_rows) and aggregated by their owner.
// The same data path as arrow_amd/parallel.py (which the driver's `bench.py --gpus N` uses through torch.distributed),
// for callers that are C++ all the way down.
//
// RCCL is resolved at the first call (dlopen "librccl.so", or the library named by ARROW_AMD_RCCL_LIBRARY), so the
// plugin itself does not depend on it: single-GPU users never load it.
struct NcclId {   // ncclUniqueId (rccl.h: 128 opaque bytes, passed by value)
  char bytes[128];
};
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(NcclId*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint8 = 1, kNcclInt64 = 4;   // ncclDataType_t (rccl.h: ncclInt8 0, ncclUint8 1, ncclInt32 2, ncclUint32 3, ncclInt64 4)

arrow::Result<const RcclApi*> Rccl() {
  static RcclApi api;
  static Status status = [] {
    const char* name = std::getenv("ARROW_AMD_RCCL_LIBRARY");
    api.handle = dlopen(name != nullptr ? name : "librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (api.handle == nullptr && name == nullptr) api.handle = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (api.handle == nullptr) return Status::IOError("arrow_amd: RCCL not found (", dlerror(), ")");
    auto sym = [&](const char* s) { return dlsym(api.handle, s); };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather || !api.Send || !api.Recv ||
        !api.GroupStart || !api.GroupEnd) {
      return Status::IOError("arrow_amd: the RCCL library lacks an entry point of the sharded group-by");
    }
    return Status::OK();
  }();
  ARROW_RETURN_NOT_OK(status);
  return &api;
}

#define RCCL_RETURN_NOT_OK(api, call)                                                                          \
  do {                                                                                                         \
    const int rc__ = (call);                                                                                   \
    if (rc__ != 0) {                                                                                           \
      return Status::IOError("RCCL: ", (api)->GetErrorString ? (api)->GetErrorString(rc__) : "error", " in " #call); \
    }                                                                                                          \
  } while (0)

struct ShardedComm {
  void* comm = nullptr;
  int world = 1, rank = 0;
};

int64_t Pow2AtLeast(int64_t x) {
  int64_t c = 16;
  while (c < x) c <<= 1;
  return c;
}

struct StageClock {
  hipStream_t st;
  double* out;
  int next = 0;
  std::chrono::steady_clock::time_point t0;
  StageClock(hipStream_t s, double* o) : st(s), out(o), t0(std::chrono::steady_clock::now()) {}
  // with stage timings asked for the stream is synchronised at every mark (diagnosis, not the timed form)
  Status Mark() {
    if (out == nullptr) return Status::OK();
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    const auto now = std::chrono::steady_clock::now();
    out[next++] = std::chrono::duration<double, std::milli>(now - t0).count();
    t0 = now;
    return Status::OK();
  }
  void Skip() {   // a stage this call did not have: exactly 0
    if (out != nullptr) out[next++] = 0.0;
  }
};

// The sharded group-by on the RANGE-PARTITIONED state (round 6; include/arrow_amd.h arx_groupby_range_*, csrc/groupby_lines.h; the
// same data path as arrow_amd/parallel.py _sharded_range_group_by_sum) — int32 keys from a narrow range, no nulls.  The owner of a
// key is the owner of its PARTITION (a slice of the key range), contiguous runs of partitions per rank:
//   1. one gather of {-min, max} of every shard's sampled keys (a shard with nulls poisons it) -> the same plan on every rank;
//   2. local consume into the rank's dense state; one gather of "my consume took its rows" (a hot key, a key the sample
//      missed: every rank then takes the table path together, nothing sent);
//   3. ONE exchange of the state itself — the run of blocks every owner gets has the same, known size on every rank;
//   4. the owner adds the P runs in one pass (Merge = vector add) and compacts its partitions' groups in key order.
// *done == false: this path does not apply (the caller goes on with the records / table path; nothing was sent but the two
// small gathers, which every rank made alike).
Status TryShardedRangeGroupBySum(const ShardedComm& c, const RcclApi* api, const ArxSpan& dk, const ArxSpan& dv, uint32_t min_count, hipStream_t st,
                                 StageClock* clock, bool* done, std::shared_ptr<ArrayData>* out_keys, std::shared_ptr<ArrayData>* out_sums) {
  *done = false;
  const int world = c.world, rank = c.rank;
  const int64_t n = dk.length;
  auto dev_ptr = [](const std::shared_ptr<Buffer>& b) { return reinterpret_cast<void*>(b->mutable_address()); };
  auto gather_i64 = [&](const int64_t* mine, int64_t count, std::vector<int64_t>* all) -> Status {
    ARROW_ASSIGN_OR_RAISE(auto d_mine, AllocDevice(count * 8));
    ARROW_ASSIGN_OR_RAISE(auto everybody, AllocDevice(count * world * 8));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(dev_ptr(d_mine), mine, static_cast<size_t>(count) * 8, hipMemcpyHostToDevice, st));
    RCCL_RETURN_NOT_OK(api, api->AllGather(dev_ptr(d_mine), dev_ptr(everybody), static_cast<size_t>(count), kNcclInt64, c.comm, st));
    all->resize(static_cast<size_t>(count) * world);
    HIP_RETURN_NOT_OK(hipMemcpyAsync(all->data(), dev_ptr(everybody), all->size() * 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    return Status::OK();
  };
  const bool nulls = dk.null_count != 0 || dv.null_count != 0;
  int64_t mine_range[2] = {int64_t(1) << 62, int64_t(1) << 62};   // {-min, max}: poisoned unless the shard qualifies
  if (!nulls && n > 0) {
    ARROW_ASSIGN_OR_RAISE(auto d_pair, AllocDevice(8));
    const int32_t init[2] = {std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
    HIP_RETURN_NOT_OK(hipMemcpyAsync(dev_ptr(d_pair), init, 8, hipMemcpyHostToDevice, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_key_range_sampled_i32(&dk, g_aggregate_range_sample_rows.load(), static_cast<int32_t*>(dev_ptr(d_pair)), st)));
    int32_t mm[2];
    HIP_RETURN_NOT_OK(hipMemcpyAsync(mm, dev_ptr(d_pair), 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    mine_range[0] = -static_cast<int64_t>(mm[0]);
    mine_range[1] = mm[1];
  } else if (!nulls) {
    mine_range[0] = -(int64_t(1) << 40);   // (an empty shard says nothing about the range)
    mine_range[1] = -(int64_t(1) << 40);
  }
  std::vector<int64_t> ranges;
  ARROW_RETURN_NOT_OK(gather_i64(mine_range, 2, &ranges));
  int64_t neg_lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::min();
  for (int r = 0; r < world; ++r) {
    neg_lo = std::max(neg_lo, ranges[2 * r]);
    hi = std::max(hi, ranges[2 * r + 1]);
  }
  const int64_t lo = -neg_lo;
  if (lo > hi || hi - lo >= (int64_t(1) << 31) || lo < std::numeric_limits<int32_t>::min() || hi > std::numeric_limits<int32_t>::max()) return Status::OK();
  // (the plan is a function of the agreed range alone: the same on every rank; the sample misses a few keys at both ends)
  const int64_t pad = (hi - lo + 1) / 64 + 1;
  const int32_t plo = static_cast<int32_t>(std::max<int64_t>(std::numeric_limits<int32_t>::min(), lo - pad));
  const int32_t phi = static_cast<int32_t>(std::min<int64_t>(std::numeric_limits<int32_t>::max(), hi + pad));
  ArxRangePlan plan{};
  const int rc_plan = arx_groupby_range_plan(1, plo, phi, &plan);
  if (rc_plan == ARX_NOT_IMPLEMENTED) return Status::OK();
  ARROW_RETURN_NOT_OK(FromArx(rc_plan));
  ArxRangePlan probe{};   // (the workspace of THIS shard's rows)
  ARROW_RETURN_NOT_OK(FromArx(arx_groupby_range_plan(std::max<int64_t>(n, 1), plan.key_min, static_cast<int32_t>(plan.key_min + plan.slots - 1), &probe)));
  ARROW_ASSIGN_OR_RAISE(auto state, AllocDevice(plan.state_bytes));
  HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(state), 0, static_cast<size_t>(plan.state_bytes), st));
  int64_t ok = 1;
  if (n > 0) {
    ARROW_ASSIGN_OR_RAISE(auto ws_buf, AllocAligned(static_cast<int64_t>(probe.workspace_bytes)));
    void* ws = ws_buf.ptr;
    const int rc = arx_groupby_range_sum_i64_consume(dev_ptr(state), &plan, &dk, &dv, ws, static_cast<size_t>(probe.workspace_bytes), st);
    if (rc == ARX_CAPACITY_ERROR || rc == ARX_NOT_IMPLEMENTED) {
      ok = 0;
    } else {
      ARROW_RETURN_NOT_OK(FromArx(rc));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the workspace goes back to the pool)
  }
  std::vector<int64_t> status;
  ARROW_RETURN_NOT_OK(gather_i64(&ok, 1, &status));
  for (int r = 0; r < world; ++r) {
    if (status[r] == 0) {
      g_sharded_range_declined.fetch_add(1);
      return Status::OK();   // (every rank sees the same status: all take the other path together)
    }
  }
  ARROW_RETURN_NOT_OK(clock->Mark());   // consume
  clock->Skip();                        // export: none
  const int64_t parts = plan.partitions, pb = static_cast<int64_t>(plan.width) * 16;
  auto run_of = [&](int r, int64_t* first, int64_t* count) {
    *first = static_cast<int64_t>(r) * parts / world;
    *count = static_cast<int64_t>(r + 1) * parts / world - *first;
  };
  int64_t first = 0, mine = 0;
  run_of(rank, &first, &mine);
  std::shared_ptr<Buffer> got = state;
  const uint8_t* blocks = static_cast<const uint8_t*>(dev_ptr(state));
  if (world > 1) {
    ARROW_ASSIGN_OR_RAISE(got, AllocDevice(std::max<int64_t>(world * mine * pb, 8)));
    RCCL_RETURN_NOT_OK(api, api->GroupStart());
    int group_rc = 0;
    for (int p = 0; p < world && group_rc == 0; ++p) {
      int64_t pf = 0, pc = 0;
      run_of(p, &pf, &pc);
      if (pc > 0) {
        group_rc = api->Send(static_cast<const uint8_t*>(dev_ptr(state)) + pf * pb, static_cast<size_t>(pc * pb), kNcclUint8, p, c.comm, st);
      }
      if (group_rc == 0 && mine > 0) {
        group_rc = api->Recv(static_cast<uint8_t*>(dev_ptr(got)) + static_cast<int64_t>(p) * mine * pb, static_cast<size_t>(mine * pb), kNcclUint8, p,
                             c.comm, st);
      }
    }
    const int end_rc = api->GroupEnd();   // (closed whatever happened: the peers would block in theirs)
    RCCL_RETURN_NOT_OK(api, group_rc);
    RCCL_RETURN_NOT_OK(api, end_rc);
    ARROW_RETURN_NOT_OK(clock->Mark());   // exchange
    if (mine > 0) {
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_range_merge(dev_ptr(got), static_cast<const uint8_t*>(dev_ptr(got)) + mine * pb, plan.width, mine,
                                                          world - 1, mine * pb, st)));
    }
    blocks = static_cast<const uint8_t*>(dev_ptr(got));
    ARROW_RETURN_NOT_OK(clock->Mark());   // merge
  } else {
    clock->Skip();   // exchange
    clock->Skip();   // merge
    first = 0;
    mine = parts;
  }
  const int64_t slots = std::max<int64_t>(mine * plan.width, 1);
  ARROW_ASSIGN_OR_RAISE(auto o_keys, AllocDevice(slots * 4));
  ARROW_ASSIGN_OR_RAISE(auto o_sums, AllocDevice(slots * 8));
  ARROW_ASSIGN_OR_RAISE(auto svalid_bytes, AllocDevice(slots));
  ARROW_ASSIGN_OR_RAISE(auto d_count, AllocDevice(8));
  HIP_RETURN_NOT_OK(hipMemsetAsync(dev_ptr(d_count), 0, 8, st));
  int64_t g = 0;
  if (mine > 0) {
    const size_t fws_bytes = arx_groupby_range_finalize_workspace_bytes(slots);
    ARROW_ASSIGN_OR_RAISE(auto fws_buf, AllocAligned(static_cast<int64_t>(fws_bytes)));
    void* fws = fws_buf.ptr;
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_range_finalize(blocks + (world > 1 ? 0 : first * pb), static_cast<int32_t>(plan.key_min + first * plan.width),
                                                           plan.width, mine, min_count, fws, fws_bytes, static_cast<int32_t*>(dev_ptr(o_keys)),
                                                           static_cast<int64_t*>(dev_ptr(o_sums)), nullptr, static_cast<uint8_t*>(dev_ptr(svalid_bytes)),
                                                           static_cast<int64_t*>(dev_ptr(d_count)), st)));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(&g, dev_ptr(d_count), 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  }
  ARROW_ASSIGN_OR_RAISE(auto sbits, AllocDevice(((g + 63) / 64) * 8 + 8));
  int64_t sum_nulls = 0;
  if (g > 0) {
    const uint8_t zero = 0;
    ARROW_RETURN_NOT_OK(FromArx(arx_compare_numeric(ARX_CMP_NOT_EQUAL, ARX_NUM_UINT8, dev_ptr(svalid_bytes), nullptr, nullptr, &zero, g,
                                                    static_cast<uint64_t*>(dev_ptr(sbits)), st)));
    ARROW_ASSIGN_OR_RAISE(sum_nulls, DeviceNullCount(*sbits, g, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  ARROW_RETURN_NOT_OK(clock->Mark());   // finalize
  *out_keys = ArrayData::Make(arrow::int32(), g, {nullptr, std::move(o_keys)}, 0);
  *out_sums = ArrayData::Make(arrow::int64(), g, {sum_nulls ? sbits : nullptr, std::move(o_sums)}, sum_nulls);
  g_sharded_range_runs.fetch_add(1);
  CountGpu(kFnHashSum);
  *done = true;
  return Status::OK();
}

// one rank's part; outputs: this rank's groups (a disjoint set of keys) as device arrays
Status ShardedGroupBySum(const ShardedComm& c, const ArrayData& keys, const ArrayData& values, bool skip_nulls, uint32_t min_count,
                         int exchange, std::shared_ptr<ArrayData>* out_keys, std::shared_ptr<ArrayData>* out_sums,
                         double* stage_ms) {
  if (keys.type->id() != Type::INT32 || values.type->id() != Type::INT64 || keys.length != values.length) {
    return Status::NotImplemented("arrow_amd sharded group-by: hash_sum(int64) GROUP BY int32 over equally long columns");
  }
  if (!DataOnRocm(keys) || !DataOnRocm(values)) return Status::Invalid("arrow_amd sharded group-by: device-resident shards");
  ARROW_ASSIGN_OR_RAISE(const RcclApi* api, Rccl());
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  StageClock clock(st, stage_ms);
  const int world = c.world;
  const int64_t n = keys.length;
  ArxSpan dk{}, dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(keys), &dk));
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(values), &dv));
  // round 6: the range-partitioned state first (keys from a narrow range, no nulls); several ranks agree on it through its
  // own small gathers, one rank alone takes it from g_sharded_range_min_rows rows
  if (exchange == 0 && g_sharded_range_state.load() && (world > 1 || n >= g_sharded_range_min_rows.load())) {
    bool done = false;
    ARROW_RETURN_NOT_OK(TryShardedRangeGroupBySum(c, api, dk, dv, min_count, st, &clock, &done, out_keys, out_sums));
    if (done) return Status::OK();
  }

  auto make_table = [&](int64_t groups_bound, std::shared_ptr<Buffer>* buf, void** state, int64_t* cap) -> Status {
    *cap = Pow2AtLeast(std::min<int64_t>(2 * groups_bound + 2, int64_t(1) << 30));
    ARROW_ASSIGN_OR_RAISE(auto table, AllocAligned(static_cast<int64_t>(arx_groupby_state_bytes(*cap))));
    *buf = std::move(table.buffer);
    *state = table.ptr;
    return FromArx(arx_groupby_init(*state, *cap, st));
  };
  auto consume = [&](void* state, int64_t cap, const ArxSpan& k, const ArxSpan& v) -> Status {
    const size_t ws_bytes = arx_groupby_consume_workspace_bytes(k.length, cap);
    AlignedDevice ws_buf{nullptr, nullptr};
    void* ws = nullptr;
    if (ws_bytes > 0) {
      ARROW_ASSIGN_OR_RAISE(ws_buf, AllocAligned(static_cast<int64_t>(ws_bytes)));
      ws = ws_buf.ptr;
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_consume(state, cap, &k, &v, ws, ws_bytes, st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the workspace goes back to the pool)
    return Status::OK();
  };

  std::shared_ptr<Buffer> owned_buf;
  void* owned = nullptr;
  int64_t owned_cap = 0;
  ARROW_ASSIGN_OR_RAISE(auto part_ws, AllocDevice(static_cast<int64_t>(arx_groupby_partition_workspace_bytes(world)) + 64));
  ARROW_ASSIGN_OR_RAISE(auto counts, AllocDevice(world * 8));
  ARROW_ASSIGN_OR_RAISE(auto all_counts, AllocDevice(static_cast<int64_t>(world) * world * 8));
  std::vector<int64_t> h_counts(static_cast<size_t>(world) * world);
  const int unit = exchange == 1 ? 16 : 24;
  std::shared_ptr<Buffer> records;
  int64_t num_records = 0;
  int64_t region_records = 0;   // > 0: the blocks lie in per-owner regions of this many records (the direct local pass)
  if (exchange == 1) {
    // ---- rows: partition the shard's rows by owner
    num_records = n;
    ARROW_ASSIGN_OR_RAISE(records, AllocDevice(std::max<int64_t>(n, 1) * 16));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_partition_rows(&dk, &dv, world, reinterpret_cast<void*>(part_ws->mutable_address()),
                                                           static_cast<size_t>(part_ws->size()),
                                                           reinterpret_cast<ArxRowRecord*>(records->mutable_address()),
                                                           reinterpret_cast<int64_t*>(counts->mutable_address()), st)));
    ARROW_RETURN_NOT_OK(clock.Mark());   // partition_rows
  } else {
    // ---- partials.  First the local pass WITHOUT a local table (round 5): the aggregate's groups leave as records in
    // the owners' regions of `records` (region p starts at p * region_records — the sends below go out of the regions as
    // they lie); shards with nulls, small shards and regions that would overflow are declined ...
    const int64_t plan_cap = Pow2AtLeast(std::min<int64_t>(2 * n + 2, int64_t(1) << 30));
    if (dk.null_count == 0 && dv.null_count == 0 && world <= 64) {
      const size_t ws_bytes = arx_groupby_consume_workspace_bytes(n, plan_cap);
      if (ws_bytes > 0) {
        ARROW_ASSIGN_OR_RAISE(auto ws_buf, AllocAligned(static_cast<int64_t>(ws_bytes)));
        void* ws = ws_buf.ptr;
        region_records = arx_groupby_partials_capacity(n, plan_cap, world);
        ARROW_ASSIGN_OR_RAISE(records, AllocDevice(region_records * world * 24));
        const int rc = arx_groupby_sum_i64_consume_partials(nullptr, plan_cap, &dk, &dv, ws, ws_bytes, world,
                                                            reinterpret_cast<ArxGroupPartial*>(records->mutable_address()), region_records,
                                                            reinterpret_cast<int64_t*>(counts->mutable_address()), st);
        if (rc == ARX_OK) {
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the workspace goes back to the pool)
          ARROW_RETURN_NOT_OK(clock.Mark());   // consume
          clock.Skip();                        // export: none
        } else if (rc == ARX_NOT_IMPLEMENTED || rc == ARX_CAPACITY_ERROR) {
          region_records = 0;
          // (ADVICE r5: the regions — ~30 bytes per row — and the scratch go back to the pool BEFORE the table path below
          //  allocates its table and its own record buffer: the fallback's peak stays what round 4's was)
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
          records.reset();
        } else {
          return FromArx(rc);
        }
      }
    }
    if (region_records == 0) {
      // ... and go through it: local aggregate, then the table's groups partitioned by owner
      std::shared_ptr<Buffer> local_buf;
      void* local = nullptr;
      int64_t local_cap = 0;
      ARROW_RETURN_NOT_OK(make_table(n, &local_buf, &local, &local_cap));
      ARROW_RETURN_NOT_OK(consume(local, local_cap, dk, dv));
      ARROW_RETURN_NOT_OK(clock.Mark());   // consume
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_num_groups(local, &num_records, st)));
      ARROW_ASSIGN_OR_RAISE(records, AllocDevice(std::max<int64_t>(num_records, 1) * 24));
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_export_partitioned(local, world, reinterpret_cast<void*>(part_ws->mutable_address()),
                                                                 static_cast<size_t>(part_ws->size()),
                                                                 reinterpret_cast<ArxGroupPartial*>(records->mutable_address()),
                                                                 reinterpret_cast<int64_t*>(counts->mutable_address()), st)));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the local table goes back to the pool)
      ARROW_RETURN_NOT_OK(clock.Mark());   // export
    }
  }
  // ---- the block sizes: everybody's `world` counts
  RCCL_RETURN_NOT_OK(api, api->AllGather(reinterpret_cast<const void*>(counts->address()),
                                         reinterpret_cast<void*>(all_counts->mutable_address()), world, kNcclInt64, c.comm, st));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(h_counts.data(), reinterpret_cast<const void*>(all_counts->address()), h_counts.size() * 8,
                                   hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  std::vector<int64_t> send(world), recv(world), soff(world + 1, 0), roff(world + 1, 0);
  for (int p = 0; p < world; ++p) {
    send[p] = h_counts[static_cast<size_t>(c.rank) * world + p];
    recv[p] = h_counts[static_cast<size_t>(p) * world + c.rank];
    soff[p + 1] = region_records > 0 ? static_cast<int64_t>(p + 1) * region_records : soff[p] + send[p];
    roff[p + 1] = roff[p] + recv[p];
  }
  const int64_t total_recv = roff[world];
  ARROW_ASSIGN_OR_RAISE(auto inbox, AllocDevice(std::max<int64_t>(total_recv, 1) * unit));
  // ---- the ONE data exchange: a send / recv pair per peer inside one group
  // (a failing send / recv must not leave the group open — the peers would block in their GroupEnd: remember the first
  //  error, close the group whatever happened, then report; ADVICE r3)
  RCCL_RETURN_NOT_OK(api, api->GroupStart());
  int group_rc = 0;
  for (int p = 0; p < world && group_rc == 0; ++p) {
    if (send[p] > 0) {
      group_rc = api->Send(reinterpret_cast<const uint8_t*>(records->address()) + soff[p] * unit,
                                        static_cast<size_t>(send[p]) * unit, kNcclUint8, p, c.comm, st);
    }
    if (group_rc == 0 && recv[p] > 0) {
      group_rc = api->Recv(reinterpret_cast<uint8_t*>(inbox->mutable_address()) + roff[p] * unit,
                                        static_cast<size_t>(recv[p]) * unit, kNcclUint8, p, c.comm, st);
    }
  }
  const int end_rc = api->GroupEnd();
  RCCL_RETURN_NOT_OK(api, group_rc);
  RCCL_RETURN_NOT_OK(api, end_rc);
  ARROW_RETURN_NOT_OK(clock.Mark());   // exchange
  // ---- the owner's side
  if (exchange == 1) {
    ARROW_RETURN_NOT_OK(make_table(total_recv, &owned_buf, &owned, &owned_cap));
    ARROW_ASSIGN_OR_RAISE(auto rk, AllocDevice(std::max<int64_t>(total_recv, 1) * 4));
    ARROW_ASSIGN_OR_RAISE(auto rv, AllocDevice(std::max<int64_t>(total_recv, 1) * 8));
    ARROW_ASSIGN_OR_RAISE(auto kb, AllocDevice(((total_recv + 63) / 64) * 8 + 8));
    ARROW_ASSIGN_OR_RAISE(auto vb, AllocDevice(((total_recv + 63) / 64) * 8 + 8));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_unpack_rows(reinterpret_cast<const ArxRowRecord*>(inbox->address()), total_recv,
                                                        reinterpret_cast<int32_t*>(rk->mutable_address()),
                                                        reinterpret_cast<int64_t*>(rv->mutable_address()),
                                                        reinterpret_cast<void*>(kb->mutable_address()),
                                                        reinterpret_cast<void*>(vb->mutable_address()), st)));
    if (total_recv > 0) {
      const ArxSpan k2{reinterpret_cast<const void*>(kb->address()), reinterpret_cast<const void*>(rk->address()), 0, total_recv, -1};
      const ArxSpan v2{reinterpret_cast<const void*>(vb->address()), reinterpret_cast<const void*>(rv->address()), 0, total_recv, -1};
      ARROW_RETURN_NOT_OK(consume(owned, owned_cap, k2, v2));
    }
    ARROW_RETURN_NOT_OK(clock.Mark());   // consume
  } else {
    ARROW_RETURN_NOT_OK(make_table(total_recv, &owned_buf, &owned, &owned_cap));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_merge_records(owned, owned_cap, reinterpret_cast<const ArxGroupPartial*>(inbox->address()),
                                                                  total_recv, st)));
    ARROW_RETURN_NOT_OK(clock.Mark());   // merge
  }
  // ---- Finalize: the owned groups as device arrays (key + validity, sum + validity)
  int64_t g = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_groupby_num_groups(owned, &g, st)));
  const int64_t g1 = std::max<int64_t>(g, 1);
  ARROW_ASSIGN_OR_RAISE(auto o_keys, AllocDevice(g1 * 4));
  ARROW_ASSIGN_OR_RAISE(auto o_sums, AllocDevice(g1 * 8));
  ARROW_ASSIGN_OR_RAISE(auto o_counts, AllocDevice(g1 * 8));
  ARROW_ASSIGN_OR_RAISE(auto kvalid_bytes, AllocDevice(g1));
  ARROW_ASSIGN_OR_RAISE(auto no_nulls, AllocDevice(g1));
  ARROW_ASSIGN_OR_RAISE(auto svalid_bytes, AllocDevice(g1));
  ARROW_ASSIGN_OR_RAISE(auto kbits, AllocDevice(((g + 63) / 64) * 8 + 8));
  ARROW_ASSIGN_OR_RAISE(auto sbits, AllocDevice(((g + 63) / 64) * 8 + 8));
  int64_t key_nulls = 0, sum_nulls = 0;
  if (g > 0) {
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_export(owned, reinterpret_cast<int32_t*>(o_keys->mutable_address()),
                                                           reinterpret_cast<uint8_t*>(kvalid_bytes->mutable_address()),
                                                           reinterpret_cast<int64_t*>(o_sums->mutable_address()),
                                                           reinterpret_cast<int64_t*>(o_counts->mutable_address()),
                                                           reinterpret_cast<uint8_t*>(no_nulls->mutable_address()), st)));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_finalize(reinterpret_cast<const int64_t*>(o_counts->address()),
                                                             reinterpret_cast<const uint8_t*>(no_nulls->address()), g, skip_nulls ? 1 : 0,
                                                             min_count, reinterpret_cast<uint8_t*>(svalid_bytes->mutable_address()), st)));
    // one validity BYTE per group -> Arrow bitmaps: byte != 0, packed by the compare kernel
    const uint8_t zero = 0;
    ARROW_RETURN_NOT_OK(FromArx(arx_compare_numeric(ARX_CMP_NOT_EQUAL, ARX_NUM_UINT8, reinterpret_cast<const void*>(kvalid_bytes->address()),
                                                    nullptr, nullptr, &zero, g, reinterpret_cast<uint64_t*>(kbits->mutable_address()), st)));
    ARROW_RETURN_NOT_OK(FromArx(arx_compare_numeric(ARX_CMP_NOT_EQUAL, ARX_NUM_UINT8, reinterpret_cast<const void*>(svalid_bytes->address()),
                                                    nullptr, nullptr, &zero, g, reinterpret_cast<uint64_t*>(sbits->mutable_address()), st)));
    ARROW_ASSIGN_OR_RAISE(key_nulls, DeviceNullCount(*kbits, g, st));
    ARROW_ASSIGN_OR_RAISE(sum_nulls, DeviceNullCount(*sbits, g, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  ARROW_RETURN_NOT_OK(clock.Mark());   // finalize
  *out_keys = ArrayData::Make(arrow::int32(), g, {key_nulls ? kbits : nullptr, std::move(o_keys)}, key_nulls);
  *out_sums = ArrayData::Make(arrow::int64(), g, {sum_nulls ? sbits : nullptr, std::move(o_sums)}, sum_nulls);
  CountGpu(kFnHashSum);
  return Status::OK();
}
