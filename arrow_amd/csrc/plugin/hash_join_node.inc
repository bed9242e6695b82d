// The hashjoin_rocm Acero exec node.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: hash join node
// HashJoinNode (acero/hash_join_node.cc) row-encodes keys and payload on the CPU, so over device-resident batches it
// reads HBM through host pointers.  This node is the C++ form of the mirror's compute.hash_join_indices / hash_join
// (DESIGN 4.17): input 0 is the probe (left) side, input 1 the build (right) side; both are accumulated whole (an
// AccumulatingNode over two inputs, plugin/acero_common.inc: nothing streams), concatenated per column in HBM, and joined by
//   key columns -> Grouper columns (booleans as bytes, utf8 / binary as length + 12-byte chunks), the chain of Grouper
//   tables (consume the build rows, look the probe rows up), arx_hash_join_key_validity, group offsets, the stable sort
//   of the build ids, probe count (the one read-back), expand, build mask and right-only tail;
//   with HashJoinNodeOptions::filter: the candidates as an inner join, the filter's fields gathered at the candidate
//   pairs (array_take), ExecuteScalarExpression over that device batch (the shim's kernels, or the device guard's
//   Status), then arx_hash_join_filter_count / _filter_compact / _flags_to_mask (one more read-back).
// Output columns are array_take of the input columns by the row pairs (null index -> null row, no bounds check) and stay
// in HBM when any input batch was device-resident; host-only inputs are uploaded and the result copied back, as
// order_by_rocm does.  The schema, the validation and the filter's binding are the reference's own HashJoinSchema.
// Row order: the contract of include/arrow_amd.h.  Registered under a NEW name.
class RocmHashJoinNode : public AccumulatingNode {
 public:
  RocmHashJoinNode(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs, std::shared_ptr<arrow::Schema> schema,
                   ac::JoinType join_type, std::vector<ac::JoinKeyCmp> key_cmp, std::unique_ptr<ac::HashJoinSchema> maps,
                   cp::Expression filter)
      : AccumulatingNode(plan, std::move(inputs), {"left", "right"}, std::move(schema)),
        join_type_(join_type), key_cmp_(std::move(key_cmp)), maps_(std::move(maps)), filter_(std::move(filter)) {}

  static bool IsKeyType(const arrow::DataType& t) {
    switch (t.id()) {
      case Type::BOOL: case Type::STRING: case Type::BINARY:
      case Type::INT8: case Type::UINT8: case Type::INT16: case Type::UINT16: case Type::INT32: case Type::UINT32:
      case Type::INT64: case Type::UINT64: case Type::FLOAT: case Type::DOUBLE: case Type::DATE32: case Type::DATE64:
      case Type::TIMESTAMP: case Type::DURATION: case Type::TIME32: case Type::TIME64: return true;
      default: return false;
    }
  }

  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                           const ac::ExecNodeOptions& options) {
    if (inputs.size() != 2) return Status::Invalid("hashjoin_rocm takes exactly two inputs (left = probe, right = build)");
    const auto* opts = dynamic_cast<const ac::HashJoinNodeOptions*>(&options);
    if (opts == nullptr) return Status::TypeError("hashjoin_rocm expects HashJoinNodeOptions");
    const auto& left = *inputs[0]->output_schema();
    const auto& right = *inputs[1]->output_schema();
    auto maps = std::make_unique<ac::HashJoinSchema>();
    if (opts->output_all) {
      ARROW_RETURN_NOT_OK(maps->Init(opts->join_type, left, opts->left_keys, right, opts->right_keys, opts->filter,
                                     opts->output_suffix_for_left, opts->output_suffix_for_right));
    } else {
      ARROW_RETURN_NOT_OK(maps->Init(opts->join_type, left, opts->left_keys, opts->left_output, right, opts->right_keys,
                                     opts->right_output, opts->filter, opts->output_suffix_for_left,
                                     opts->output_suffix_for_right));
    }
    const int num_keys = maps->proj_maps[0].num_cols(ac::HashJoinProjection::KEY);
    if (num_keys == 0 || num_keys != maps->proj_maps[1].num_cols(ac::HashJoinProjection::KEY)) {
      return Status::Invalid("hashjoin_rocm: the same positive number of key columns on both sides is required");
    }
    for (int k = 0; k < num_keys; ++k) {
      const auto& lt = maps->proj_maps[0].data_type(ac::HashJoinProjection::KEY, k);
      const auto& rt = maps->proj_maps[1].data_type(ac::HashJoinProjection::KEY, k);
      if (!lt->Equals(*rt)) {
        return Status::Invalid("Mismatched data types for corresponding join field keys: ", lt->ToString(), " vs ", rt->ToString());
      }
      if (!IsKeyType(*lt)) {
        return Status::NotImplemented("arrow_amd: hashjoin_rocm: join keys of type ", lt->ToString(),
                                      " on device-resident data are not supported");
      }
    }
    for (int side = 0; side < 2; ++side) {
      for (auto proj : {ac::HashJoinProjection::OUTPUT, ac::HashJoinProjection::FILTER}) {
        for (int c = 0; c < maps->proj_maps[side].num_cols(proj); ++c) {
          const auto& t = *maps->proj_maps[side].data_type(proj, c);
          if (FixedByteWidth(t) == 0 && t.id() != Type::BOOL && !IsInt32Binary(t)) {
            return Status::NotImplemented("arrow_amd: hashjoin_rocm: columns of type ", t.ToString(),
                                          " on device-resident data are not gathered by the device take");
          }
        }
      }
    }
    std::vector<ac::JoinKeyCmp> cmp = opts->key_cmp;
    if (cmp.empty()) cmp.assign(num_keys, ac::JoinKeyCmp::EQ);
    if (static_cast<int>(cmp.size()) != num_keys) return Status::Invalid("key_cmp and keys must have the same size");
    cp::Expression filter = opts->filter;
    if (filter != cp::literal(true)) {
      ARROW_ASSIGN_OR_RAISE(filter, maps->BindFilter(filter, left, right, plan->query_context()->exec_context()));
    }
    auto schema = maps->MakeOutputSchema(opts->output_suffix_for_left, opts->output_suffix_for_right);
    return plan->EmplaceNode<RocmHashJoinNode>(plan, std::move(inputs), std::move(schema), opts->join_type, std::move(cmp),
                                               std::move(maps), std::move(filter));
  }

  const char* kind_name() const override { return "RocmHashJoinNode"; }

 private:
  using BufferPtr = std::shared_ptr<Buffer>;
  static bool EmitsLeft(ac::JoinType t) { return t != ac::JoinType::RIGHT_SEMI && t != ac::JoinType::RIGHT_ANTI; }
  static bool EmitsRight(ac::JoinType t) { return t != ac::JoinType::LEFT_SEMI && t != ac::JoinType::LEFT_ANTI; }

  // Key columns of both sides as the Grouper's fixed-width columns, the same widths on both sides (the mirror's
  // _join_key_columns): strings as (length, 12-byte chunks), the shorter side's missing chunks zero.
  Status KeyColumns(const std::vector<std::shared_ptr<ArrayData>> keys[2], const int64_t n[2], hipStream_t st,
                    std::vector<KeyColumn> out[2]) {
    for (size_t k = 0; k < keys[0].size(); ++k) {
      const auto& t = *keys[0][k]->type;
      if (IsInt32Binary(t)) {
        int64_t max_len[2] = {0, 0};
        ArxBinarySpan bs[2];
        KeyColumn lengths[2];
        for (int s = 0; s < 2; ++s) {
          ARROW_RETURN_NOT_OK(DeviceBinarySpan(ArraySpan(*keys[s][k]), &bs[s]));
          ARROW_ASSIGN_OR_RAISE(lengths[s], BinaryKeyLengths(bs[s], n[s], st, &max_len[s]));
        }
        for (int s = 0; s < 2; ++s) {
          ARROW_RETURN_NOT_OK(BinaryKeyColumns(bs[s], n[s], std::move(lengths[s]), std::max(max_len[0], max_len[1]), st, &out[s]));
        }
      } else {
        for (int s = 0; s < 2; ++s) {
          ArxSpan sp{};
          ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(*keys[s][k]), &sp));
          if (t.id() == Type::BOOL) {
            ARROW_ASSIGN_OR_RAISE(auto bytes, AllocDevice(std::max<int64_t>(sp.offset + n[s], 1)));
            ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_bool_key(&sp, DevPtr<uint8_t>(bytes) + sp.offset, st)));
            sp.data = DevPtr<void>(bytes);
            out[s].push_back(KeyColumn{sp, 1, false, {bytes}});
          } else {
            out[s].push_back(KeyColumn{sp, FixedByteWidth(t), false, {}});
          }
        }
      }
    }
    if (out[0].size() > 32) return Status::NotImplemented("arrow_amd: hashjoin_rocm: key rows of more than 32 Grouper columns on device-resident data");
    return Status::OK();
  }

  static arrow::Datum IndexDatum(const std::shared_ptr<arrow::DataType>& type, int64_t n, BufferPtr valid, BufferPtr data) {
    const int64_t nulls = valid != nullptr ? arrow::kUnknownNullCount : 0;
    return arrow::Datum(ArrayData::Make(type, n, {std::move(valid), std::move(data)}, nulls));
  }

  // the rows whose bit is set in `mask` (n bits), ascending: uint64
  static arrow::Result<std::shared_ptr<ArrayData>> RowsOfMask(BufferPtr mask, int64_t n, cp::ExecContext* ctx) {
    if (n == 0) return ArrayData::Make(arrow::uint64(), 0, {nullptr, mask}, 0);
    ARROW_ASSIGN_OR_RAISE(arrow::Datum rows, cp::CallFunction("indices_nonzero", {IndexDatum(arrow::boolean(), n, nullptr, std::move(mask))}, ctx));
    return rows.array();
  }

  Status Finish() override {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    cp::ExecContext* ctx = plan_->query_context()->exec_context();
    using Proj = ac::HashJoinProjection;
    const int jt = static_cast<int>(join_type_);
    int64_t n[2] = {0, 0};
    bool any_device = false;
    for (int s = 0; s < 2; ++s) {
      OrderBatchesByIndex(&batches_[s]);
      for (const auto& b : batches_[s]) n[s] += b.length;
    }
    // every input column that the keys, the filter or the output read, concatenated once
    std::map<int, std::shared_ptr<ArrayData>> whole[2];
    auto column = [&](int side, int input_col) -> arrow::Result<std::shared_ptr<ArrayData>> {
      auto it = whole[side].find(input_col);
      if (it != whole[side].end()) return it->second;
      ARROW_ASSIGN_OR_RAISE(auto col, WholeColumn(batches_[side], inputs_[side]->output_schema()->field(input_col)->type(), input_col, st,
                                                  &any_device, "arrow_amd: hashjoin_rocm"));
      whole[side][input_col] = col;
      return col;
    };
    std::vector<std::shared_ptr<ArrayData>> keys[2];
    for (int s = 0; s < 2; ++s) {
      const auto to_input = maps_->proj_maps[s].map(Proj::KEY, Proj::INPUT);
      for (int k = 0; k < maps_->proj_maps[s].num_cols(Proj::KEY); ++k) {
        ARROW_ASSIGN_OR_RAISE(auto col, column(s, to_input.get(k)));
        keys[s].push_back(std::move(col));
      }
    }
    const int64_t nl = n[0], nb = n[1];
    std::vector<KeyColumn> key_cols[2];
    ARROW_RETURN_NOT_OK(KeyColumns(keys, n, st, key_cols));
    ARROW_ASSIGN_OR_RAISE(GrouperChain chain, GrouperChain::Make(PlanGrouperLevels(key_cols[1]), nb, st));
    BufferPtr build_ids, probe_ids, probe_found;
    ARROW_RETURN_NOT_OK(chain.Run(key_cols[1], nb, /*lookup=*/false, st, &build_ids, nullptr));
    ARROW_RETURN_NOT_OK(chain.Run(key_cols[0], nl, /*lookup=*/true, st, &probe_ids, &probe_found));
    const int64_t num_groups = chain.num_groups;
    // JoinKeyCmp::EQ: a null key matches nothing; IS: null is the Grouper's key value of its own
    BufferPtr valid[2];
    for (int s = 0; s < 2; ++s) {
      std::vector<ArxSpan> spans;
      if (s == 0) spans.push_back(ArxSpan{DevPtr<void>(probe_found), DevPtr<void>(probe_ids), 0, nl, arrow::kUnknownNullCount});
      for (size_t k = 0; k < keys[s].size(); ++k) {
        if (key_cmp_[k] != ac::JoinKeyCmp::EQ || keys[s][k]->buffers[0] == nullptr) continue;
        spans.push_back(ArxSpan{reinterpret_cast<const void*>(keys[s][k]->buffers[0]->address()), nullptr, keys[s][k]->offset, n[s],
                                arrow::kUnknownNullCount});
      }
      if (spans.empty() || n[s] == 0) continue;
      ARROW_ASSIGN_OR_RAISE(valid[s], AllocDevice(BitmapBytes(n[s])));
      ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_key_validity(spans.data(), static_cast<int>(spans.size()), n[s], DevPtr<void>(valid[s]), st)));
    }
    const BufferPtr &probe_valid = valid[0], &build_valid = valid[1];

    const size_t ws_bytes = arx_hash_join_workspace_bytes(std::max<int64_t>({num_groups, nl, 1}));
    ARROW_ASSIGN_OR_RAISE(auto ws, AllocDevice(static_cast<int64_t>(ws_bytes) + 64));
    ARROW_ASSIGN_OR_RAISE(auto group_offsets, AllocDevice((num_groups + 1) * 8));
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_group_offsets(DevPtr<uint32_t>(build_ids), DevPtr<void>(build_valid), nb, num_groups,
                                                            DevPtr<int64_t>(group_offsets), DevPtr<void>(ws), ws_bytes, st)));
    ARROW_ASSIGN_OR_RAISE(auto offsets, AllocDevice((nl + 1) * 8));
    // rows the output (and, under a filter, the candidate pairs) may have before the join is refused with a
    // CapacityError: 2^33 rows are 146 GB of row pairs and bitmap, half of the MI355X's HBM before a column is gathered
    const int64_t limit = int64_t(1) << 33;
    const bool filtered = filter_ != cp::literal(true);
    const bool right_side = jt == 1 || jt == 3 || jt == 6 || jt == 7;
    const bool pairs = jt >= 4;
    auto sorted_build_rows = [&]() -> arrow::Result<BufferPtr> {
      const cp::ArraySortOptions sort_options(cp::SortOrder::Ascending, cp::NullPlacement::AtEnd);
      ARROW_ASSIGN_OR_RAISE(arrow::Datum sorted, cp::CallFunction("array_sort_indices", {IndexDatum(arrow::uint32(), nb, build_valid, build_ids)},
                                                                   &sort_options, ctx));
      if (sorted.array()->offset != 0) return Status::Invalid("arrow_amd: hashjoin_rocm: sorted build rows with an offset");
      return sorted.array()->buffers[1];
    };
    auto too_many = [&](int64_t n_out) {
      return Status::CapacityError("hash join: the output would have ", n_out, " rows, more than the ", limit, " that can be allocated");
    };

    arrow::Datum left_rows, right_rows;   // the row pairs: int64 with validity, or uint64 rows of one side (semi / anti)
    int64_t n_out = 0;
    // the row pairs of the joins that emit probe rows: size the output, allocate the pair and validity buffers, `fill` them
    // (expand, or compact under a filter), append the right-only tail, wrap as index Datums (compute.py _PreparedJoin.finish)
    using Fill = std::function<Status(const BufferPtr& out_left, const BufferPtr& out_right, const BufferPtr& right_valid)>;
    auto row_pairs = [&](int64_t total, const std::shared_ptr<ArrayData>& tail, const Fill& fill) -> Status {
      n_out = total + (tail != nullptr ? tail->length : 0);
      if (n_out > limit) return too_many(n_out);
      BufferPtr out_left, out_right, right_valid, left_valid;
      ARROW_ASSIGN_OR_RAISE(out_left, AllocDevice(std::max<int64_t>(n_out, 1) * 8));
      if (pairs) {
        ARROW_ASSIGN_OR_RAISE(out_right, AllocDevice(std::max<int64_t>(n_out, 1) * 8));
      }
      if (jt == 5 || jt == 7) {
        ARROW_ASSIGN_OR_RAISE(right_valid, AllocDevice(BitmapBytes(n_out)));
      }
      ARROW_RETURN_NOT_OK(fill(out_left, out_right, right_valid));
      if (tail != nullptr && tail->length > 0) {
        ARROW_ASSIGN_OR_RAISE(left_valid, AllocDevice(BitmapBytes(n_out)));
        ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_append_build_rows(reinterpret_cast<const uint64_t*>(tail->buffers[1]->address()) + tail->offset, tail->length,
                                                                    total, DevPtr<int64_t>(out_left), DevPtr<void>(left_valid), DevPtr<int64_t>(out_right),
                                                                    DevPtr<void>(right_valid), st)));
      }
      left_rows = IndexDatum(arrow::int64(), n_out, left_valid, out_left);
      if (pairs) right_rows = IndexDatum(arrow::int64(), n_out, right_valid, out_right);
      return Status::OK();
    };
    if (!filtered) {
      BufferPtr matched;
      if (right_side) {
        ARROW_ASSIGN_OR_RAISE(matched, ZeroedDevice(std::max<int64_t>(num_groups, 1), st));
      }
      int64_t total = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_probe_count(DevPtr<uint32_t>(probe_ids), DevPtr<void>(probe_valid), nl, DevPtr<int64_t>(group_offsets), num_groups, jt,
                                                            DevPtr<uint8_t>(matched), limit, DevPtr<int64_t>(offsets), DevPtr<void>(ws), ws_bytes, &total, st)));
      auto build_rows = [&](int want_matched) -> arrow::Result<std::shared_ptr<ArrayData>> {
        ARROW_ASSIGN_OR_RAISE(auto mask, ZeroedDevice(BitmapBytes(nb), st));
        ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_build_mask(DevPtr<uint32_t>(build_ids), DevPtr<void>(build_valid), nb, DevPtr<uint8_t>(matched), want_matched,
                                                             DevPtr<void>(mask), st)));
        return RowsOfMask(std::move(mask), nb, ctx);
      };
      if (jt == 1 || jt == 3) {
        ARROW_ASSIGN_OR_RAISE(auto rows, build_rows(jt == 1 ? 1 : 0));
        n_out = rows->length;
        right_rows = arrow::Datum(rows);
      } else {
        std::shared_ptr<ArrayData> tail;
        if (jt == 6 || jt == 7) {
          ARROW_ASSIGN_OR_RAISE(tail, build_rows(0));
        }
        ARROW_RETURN_NOT_OK(row_pairs(total, tail, [&](const BufferPtr& out_left, const BufferPtr& out_right, const BufferPtr& right_valid) -> Status {
          BufferPtr sorted_rows;
          if (pairs && total > 0) {
            ARROW_ASSIGN_OR_RAISE(sorted_rows, sorted_build_rows());
          }
          return FromArx(arx_hash_join_expand(DevPtr<int64_t>(offsets), DevPtr<uint32_t>(probe_ids), DevPtr<void>(probe_valid), nl, DevPtr<int64_t>(group_offsets),
                                              DevPtr<uint64_t>(sorted_rows), jt, total, DevPtr<int64_t>(out_left), DevPtr<int64_t>(out_right),
                                              DevPtr<void>(right_valid), st));
        }));
      }
    } else {
      // the candidates as an inner join
      int64_t T = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_probe_count(DevPtr<uint32_t>(probe_ids), DevPtr<void>(probe_valid), nl, DevPtr<int64_t>(group_offsets), num_groups, 4,
                                                            nullptr, limit, DevPtr<int64_t>(offsets), DevPtr<void>(ws), ws_bytes, &T, st)));
      ARROW_ASSIGN_OR_RAISE(auto cand_left, AllocDevice(std::max<int64_t>(T, 1) * 8));
      ARROW_ASSIGN_OR_RAISE(auto cand_right, AllocDevice(std::max<int64_t>(T, 1) * 8));
      ArxSpan pass{nullptr, nullptr, 0, 0, 0};
      std::shared_ptr<ArrayData> pass_data;
      BufferPtr constant_pass;
      if (T > 0) {
        ARROW_ASSIGN_OR_RAISE(auto sorted_rows, sorted_build_rows());
        ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_expand(DevPtr<int64_t>(offsets), DevPtr<uint32_t>(probe_ids), DevPtr<void>(probe_valid), nl, DevPtr<int64_t>(group_offsets),
                                                         DevPtr<uint64_t>(sorted_rows), 4, T, DevPtr<int64_t>(cand_left), DevPtr<int64_t>(cand_right), nullptr, st)));
        // the fields the filter reads, gathered at the candidate pairs: left fields, then right fields (BindFilter's schema)
        const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
        std::vector<arrow::Datum> values;
        for (int s = 0; s < 2; ++s) {
          const auto to_input = maps_->proj_maps[s].map(Proj::FILTER, Proj::INPUT);
          const arrow::Datum rows = IndexDatum(arrow::int64(), T, nullptr, s == 0 ? cand_left : cand_right);
          for (int c = 0; c < maps_->proj_maps[s].num_cols(Proj::FILTER); ++c) {
            ARROW_ASSIGN_OR_RAISE(auto col, column(s, to_input.get(c)));
            ARROW_ASSIGN_OR_RAISE(arrow::Datum taken, cp::CallFunction("array_take", {arrow::Datum(col), rows}, &no_check, ctx));
            values.push_back(std::move(taken));
          }
        }
        ARROW_ASSIGN_OR_RAISE(arrow::Datum result, cp::ExecuteScalarExpression(filter_, cp::ExecBatch(std::move(values), T), ctx));
        if (result.type() == nullptr || result.type()->id() != Type::BOOL) return Status::Invalid("arrow_amd: hashjoin_rocm: the filter is not boolean");
        if (result.is_scalar()) {   // a constant filter: every candidate passes, or none
          const auto& flag = result.scalar_as<arrow::BooleanScalar>();
          ARROW_ASSIGN_OR_RAISE(constant_pass, AllocDevice(BitmapBytes(T)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(DevPtr<void>(constant_pass), flag.is_valid && flag.value ? 0xFF : 0, static_cast<size_t>(BitmapBytes(T)), st));
          pass = ArxSpan{nullptr, DevPtr<void>(constant_pass), 0, T, 0};
        } else {
          pass_data = result.array();
          if (pass_data->length != T) return Status::Invalid("arrow_amd: hashjoin_rocm: the filter's result has the wrong length");
          if (!DataOnRocm(*pass_data)) return Status::NotImplemented("arrow_amd: hashjoin_rocm: a filter over device-resident columns that evaluates on the host");
          ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(*pass_data), &pass));
        }
      }
      const int64_t words = (T + 63) / 64;
      BufferPtr build_hit, probe_hit;
      if (right_side) {
        ARROW_ASSIGN_OR_RAISE(build_hit, ZeroedDevice(std::max<int64_t>(nb, 1), st));
      }
      if (jt == 0 || jt == 2) {
        ARROW_ASSIGN_OR_RAISE(probe_hit, AllocDevice(std::max<int64_t>(nl, 1)));
      }
      ARROW_ASSIGN_OR_RAISE(auto pass_bits, AllocDevice(std::max<int64_t>(words, 1) * 8));
      ARROW_ASSIGN_OR_RAISE(auto prefix, AllocDevice((words + 1) * 8));
      ARROW_ASSIGN_OR_RAISE(auto new_offsets, AllocDevice((nl + 1) * 8));
      const size_t fws_bytes = arx_hash_join_workspace_bytes(std::max<int64_t>({nl, words, 1}));
      ARROW_ASSIGN_OR_RAISE(auto fws, AllocDevice(static_cast<int64_t>(fws_bytes) + 64));
      int64_t total = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_filter_count(&pass, DevPtr<int64_t>(offsets), DevPtr<int64_t>(cand_right), nl, jt, DevPtr<uint8_t>(build_hit),
                                                             DevPtr<uint8_t>(probe_hit), limit, DevPtr<void>(pass_bits), DevPtr<int64_t>(prefix),
                                                             DevPtr<int64_t>(new_offsets), DevPtr<void>(fws), fws_bytes, &total, st)));
      auto rows_of_flags = [&](const BufferPtr& flags, int64_t count, int want_set) -> arrow::Result<std::shared_ptr<ArrayData>> {
        ARROW_ASSIGN_OR_RAISE(auto mask, ZeroedDevice(BitmapBytes(count), st));
        ARROW_RETURN_NOT_OK(FromArx(arx_hash_join_flags_to_mask(DevPtr<uint8_t>(flags), count, want_set, DevPtr<void>(mask), st)));
        return RowsOfMask(std::move(mask), count, ctx);
      };
      if (jt == 0 || jt == 2) {
        ARROW_ASSIGN_OR_RAISE(auto rows, rows_of_flags(probe_hit, nl, jt == 0 ? 1 : 0));
        n_out = rows->length;
        left_rows = arrow::Datum(rows);
      } else if (jt == 1 || jt == 3) {
        ARROW_ASSIGN_OR_RAISE(auto rows, rows_of_flags(build_hit, nb, jt == 1 ? 1 : 0));
        n_out = rows->length;
        right_rows = arrow::Datum(rows);
      } else {
        std::shared_ptr<ArrayData> tail;
        if (jt == 6 || jt == 7) {
          ARROW_ASSIGN_OR_RAISE(tail, rows_of_flags(build_hit, nb, 0));
        }
        ARROW_RETURN_NOT_OK(row_pairs(total, tail, [&](const BufferPtr& out_left, const BufferPtr& out_right, const BufferPtr& right_valid) -> Status {
          return FromArx(arx_hash_join_filter_compact(DevPtr<void>(pass_bits), DevPtr<int64_t>(prefix), T, DevPtr<int64_t>(offsets), DevPtr<int64_t>(new_offsets), nl,
                                                      DevPtr<int64_t>(cand_left), DevPtr<int64_t>(cand_right), jt, total, DevPtr<int64_t>(out_left),
                                                      DevPtr<int64_t>(out_right), DevPtr<void>(right_valid), st));
        }));
      }
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (pass_data and the candidates are released below)
    }

    // output columns: left then right, array_take by the row pairs (null index -> null row)
    const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
    std::vector<arrow::Datum> out_columns;
    for (int s = 0; s < 2; ++s) {
      if (s == 0 ? !EmitsLeft(join_type_) : !EmitsRight(join_type_)) continue;
      const auto to_input = maps_->proj_maps[s].map(Proj::OUTPUT, Proj::INPUT);
      const arrow::Datum& rows = s == 0 ? left_rows : right_rows;
      for (int c = 0; c < maps_->proj_maps[s].num_cols(Proj::OUTPUT); ++c) {
        ARROW_ASSIGN_OR_RAISE(auto col, column(s, to_input.get(c)));
        ARROW_ASSIGN_OR_RAISE(arrow::Datum taken, cp::CallFunction("array_take", {arrow::Datum(col), rows}, &no_check, ctx));
        out_columns.push_back(std::move(taken));
      }
    }
    if (static_cast<int>(out_columns.size()) != output_schema_->num_fields()) {
      return Status::Invalid("arrow_amd: hashjoin_rocm: ", out_columns.size(), " output columns for a schema of ", output_schema_->num_fields());
    }
    batches_[0].clear();
    batches_[1].clear();
    whole[0].clear();
    whole[1].clear();
    CountGpu(kFnHashJoin);
    return EmitResult(this, output_, std::move(out_columns), n_out, any_device, st);
  }

  const ac::JoinType join_type_;
  const std::vector<ac::JoinKeyCmp> key_cmp_;
  const std::unique_ptr<ac::HashJoinSchema> maps_;
  const cp::Expression filter_;
};
