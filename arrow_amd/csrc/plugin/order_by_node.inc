// The order_by_rocm Acero exec node.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: order-by node
// OrderByNode (acero/order_by_node.cc:45-150) accumulates every batch, builds a Table, calls
// SortIndices(table) and Take(table, indices) and re-slices the result into batches.  Its table sorter and its
// chunked Take walk buffers on the CPU (vector_sort.cc TableSorter; TakeCA concatenates,
// vector_selection_take_internal.cc:542-552), so it cannot run over kROCM batches.  This node does the same
// three steps with the data in HBM:
//   1. Concatenate per column (array/concatenate.cc): bytes by memcpy, bitmaps appended at bit granularity
//      (arx_bitmap_copy_at), utf8/binary offsets rebased (arx_binary_rebase_offsets); chunks that are
//      consecutive slices of one device array (a device table cut up by table_source) are re-joined for free;
//   2. one stable device sort per sort key, least-significant key first, composed with take
//      (perm = take(perm, sort(take(key, perm)))) — the lexicographic stable order of the table sorter, each key
//      with its own direction and null placement (compute/ordering.h:50-61);
//   3. array_take of every column by the permutation.
// Steps 2 and 3 go through CallFunction, i.e. through the kernels this shim registered.  Host batches are
// uploaded by step 1 and the result is copied back, so the node is a drop-in for "order_by" either way.
// Step 1 and the way out (slices, numbers, exact null counts) are WholeColumn / EmitResult of plugin/acero_common.inc.
// Registered under a NEW name (duplicates are rejected, acero/exec_plan.cc:1132-1142).
// Lexicographic stable sort over several device-resident key columns (what TableSorter / MultipleKeyRecordBatchSorter,
// kernels/vector_sort.cc:850-954, compute on the CPU): least-significant key first, one stable device sort per key,
// composed with take — perm = sort(k_last); perm = take(perm, sort(take(k, perm))) for each earlier key.  Every step
// is a registered kernel (array_sort_indices / array_take) reached through CallFunction.
struct DeviceSortKey {
  arrow::Datum column;   // one array, buffers in HBM
  cp::SortOrder order;
  cp::NullPlacement placement;
};

// A decimal128 key column as the two keys it is: (high word, int64) before (low word, uint64) — arx_dec128_split; both halves
// share the column's validity (copied to bit 0) and its order / null placement
arrow::Result<std::pair<arrow::Datum, arrow::Datum>> SplitDecimalKeyOnDevice(const ArrayData& column) {
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(column), &dv));
  const int64_t n = column.length;
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> lo, AllocDevice(std::max<int64_t>(n, 1) * 8));
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> hi, AllocDevice(std::max<int64_t>(n, 1) * 8));
  std::shared_ptr<Buffer> bits;
  if (n > 0) {
    ARROW_RETURN_NOT_OK(FromArx(arx_dec128_split(static_cast<const uint8_t*>(dv.data) + dv.offset * 16, n,
                                                 reinterpret_cast<uint64_t*>(lo->mutable_address()), reinterpret_cast<uint64_t*>(hi->mutable_address()), st)));
    if (dv.validity != nullptr) {
      ARROW_ASSIGN_OR_RAISE(bits, AllocDevice(((n + 63) / 64) * 8 + 8));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv.validity, dv.offset, n, reinterpret_cast<void*>(bits->mutable_address()), st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  }
  const int64_t nulls = bits != nullptr ? arrow::kUnknownNullCount : 0;
  return std::make_pair(arrow::Datum(ArrayData::Make(arrow::int64(), n, {bits, hi}, nulls)),
                        arrow::Datum(ArrayData::Make(arrow::uint64(), n, {bits, lo}, nulls)));
}

// A utf8 / binary key column as the keys it is: chunk 0, chunk 1, ... (8 bytes each, big-endian: arx_binary_sort_chunk), then
// the length — bytewise lexicographic order, the shorter string first on a common prefix.  Strings of more than
// kMaxSortKeyBytes bytes are refused (every 8 bytes are one more stable sort of all rows).
constexpr int64_t kMaxSortKeyBytes = 256;
arrow::Result<std::vector<arrow::Datum>> SplitBinaryKeyOnDevice(const ArrayData& column) {
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxBinarySpan dv{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(ArraySpan(column), &dv));
  const int64_t n = column.length;
  std::vector<arrow::Datum> out;
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> lengths, AllocDevice(std::max<int64_t>(n, 1) * 4));
  int64_t max_len = 0;
  std::shared_ptr<Buffer> bits;
  if (n > 0) {
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &ws));
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_key_lengths(&dv, reinterpret_cast<uint32_t*>(lengths->mutable_address()), &max_len, ws, st)));
    if (max_len > kMaxSortKeyBytes) {
      return Status::NotImplemented("arrow_amd: sort key strings of up to ", kMaxSortKeyBytes, " bytes on device-resident data (longest here: ", max_len, ")");
    }
    if (dv.validity != nullptr) {
      ARROW_ASSIGN_OR_RAISE(bits, AllocDevice(((n + 63) / 64) * 8 + 8));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv.validity, dv.offset, n, reinterpret_cast<void*>(bits->mutable_address()), st)));
    }
  }
  const int64_t nulls = bits != nullptr ? arrow::kUnknownNullCount : 0;
  for (int64_t c = 0; c * 8 < max_len; ++c) {
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> chunk, AllocDevice(std::max<int64_t>(n, 1) * 8));
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_sort_chunk(&dv, c, reinterpret_cast<uint64_t*>(chunk->mutable_address()), st)));
    out.push_back(arrow::Datum(ArrayData::Make(arrow::uint64(), n, {bits, chunk}, nulls)));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  out.push_back(arrow::Datum(ArrayData::Make(arrow::uint32(), n, {bits, lengths}, nulls)));
  return out;
}

// large_utf8 / large_binary sort keys (round 6): the column's int64 offsets narrowed to int32 on the device when its bytes
// allow it (the last offset below 2^31: read back, 8 bytes), then the utf8 / binary chain above.  The narrowed array starts
// at row 0: its n + 1 offsets are cast from the column's slice, its validity copied to bit 0; the data buffer is shared.
arrow::Result<std::shared_ptr<ArrayData>> NarrowLargeBinaryOnDevice(const ArrayData& column) {
  const int64_t n = column.length;
  const bool utf8 = column.type->id() == Type::LARGE_STRING;
  auto narrow_type = utf8 ? arrow::utf8() : arrow::binary();
  if (column.buffers.size() < 3 || column.buffers[1] == nullptr) return Status::Invalid("arrow_amd: a large binary array without offsets");
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  const auto* offsets = reinterpret_cast<const int64_t*>(column.buffers[1]->address()) + column.offset;
  int64_t last = 0;
  HIP_RETURN_NOT_OK(hipMemcpyAsync(&last, offsets + n, 8, hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  if (last > std::numeric_limits<int32_t>::max()) {
    return Status::NotImplemented("arrow_amd: ", column.type->ToString(), " sort keys over more than 2^31 - 1 bytes of device-resident data");
  }
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> narrow, AllocDevice((n + 1) * 4));
  ArxSpan wide{nullptr, offsets, 0, n + 1, 0};
  void* flag = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &flag));
  ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&wide, ARX_NUM_INT64, ARX_NUM_INT32, /*allow_int_overflow=*/1, /*allow_float_truncate=*/1, flag, 64,
                                               reinterpret_cast<void*>(narrow->mutable_address()), st)));
  std::shared_ptr<Buffer> bits;
  if (column.buffers[0] != nullptr) {
    ARROW_ASSIGN_OR_RAISE(bits, AllocDevice(((n + 63) / 64) * 8 + 8));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(reinterpret_cast<const void*>(column.buffers[0]->address()), column.offset, n,
                                                reinterpret_cast<void*>(bits->mutable_address()), st)));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  const int64_t nulls = bits != nullptr ? arrow::kUnknownNullCount : 0;
  return ArrayData::Make(std::move(narrow_type), n, {std::move(bits), std::move(narrow), column.buffers[2]}, nulls);
}

bool IsDeviceSortKeyType(const arrow::DataType& t) {
  switch (t.id()) {
    case Type::STRING: case Type::BINARY:
    case Type::DECIMAL128: case Type::BOOL: case Type::DICTIONARY:
    case Type::INT8: case Type::UINT8: case Type::INT16: case Type::UINT16:
    case Type::UINT64: case Type::INT64: case Type::UINT32: case Type::INT32: case Type::DOUBLE: case Type::FLOAT:
    case Type::DATE32: case Type::DATE64: case Type::TIMESTAMP: case Type::DURATION: case Type::TIME32:
    case Type::TIME64: return true;
    default: return false;
  }
}

arrow::Result<arrow::Datum> SortIndicesByKeysOnDevice(const std::vector<DeviceSortKey>& given, cp::ExecContext* ctx) {
  if (given.empty()) return Status::Invalid("Must specify one or more sort keys");
  std::vector<DeviceSortKey> keys;
  for (const DeviceSortKey& k : given) {
    if (k.column.type()->id() == Type::DECIMAL128 && k.column.is_array()) {
      ARROW_ASSIGN_OR_RAISE(auto halves, SplitDecimalKeyOnDevice(*k.column.array()));
      keys.push_back(DeviceSortKey{halves.first, k.order, k.placement});
      keys.push_back(DeviceSortKey{halves.second, k.order, k.placement});
    } else if ((k.column.type()->id() == Type::STRING || k.column.type()->id() == Type::BINARY) && k.column.is_array()) {
      ARROW_ASSIGN_OR_RAISE(auto parts, SplitBinaryKeyOnDevice(*k.column.array()));
      for (auto& part : parts) keys.push_back(DeviceSortKey{std::move(part), k.order, k.placement});
    } else if (BinaryOffsetWidth(k.column.type()->id()) == 8 && k.column.is_array()) {
      ARROW_ASSIGN_OR_RAISE(auto narrowed, NarrowLargeBinaryOnDevice(*k.column.array()));
      ARROW_ASSIGN_OR_RAISE(auto parts, SplitBinaryKeyOnDevice(*narrowed));
      for (auto& part : parts) keys.push_back(DeviceSortKey{std::move(part), k.order, k.placement});
    } else {
      keys.push_back(k);
    }
  }
  const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
  arrow::Datum perm;
  for (auto it = keys.rbegin(); it != keys.rend(); ++it) {
    if (!IsDeviceSortKeyType(*it->column.type())) {
      return Status::NotImplemented("arrow_amd: sort key of type ", it->column.type()->ToString(), " on device-resident data");
    }
    const cp::ArraySortOptions sort_options(it->order, it->placement);
    if (perm.kind() == arrow::Datum::NONE) {
      ARROW_ASSIGN_OR_RAISE(perm, cp::CallFunction("array_sort_indices", {it->column}, &sort_options, ctx));
    } else {
      ARROW_ASSIGN_OR_RAISE(auto key, cp::CallFunction("array_take", {it->column, perm}, &no_check, ctx));
      ARROW_ASSIGN_OR_RAISE(auto step, cp::CallFunction("array_sort_indices", {key}, &sort_options, ctx));
      ARROW_ASSIGN_OR_RAISE(perm, cp::CallFunction("array_take", {perm, step}, &no_check, ctx));
    }
  }
  return perm;
}

// array_sort_indices of a device-resident decimal128 / utf8 / binary array (declared in plugin/sort.inc, slots 16 - 18)
Status DecimalSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out) {
  std::vector<DeviceSortKey> keys{DeviceSortKey{arrow::Datum(values.ToArrayData()), options.order, options.null_placement}};
  ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, SortIndicesByKeysOnDevice(keys, ctx));
  out->buffers[1] = perm.array()->buffers[1];
  return Status::OK();
}

// array_sort_indices of a device-resident boolean array (declared in plugin/sort.inc, slot 19): the reference's counting sort
// (ArrayCountSorter<BooleanType>, vector_array_sort.cc:360-400) — falses, trues (or trues, falses: descending) and the nulls
// at their end, every class in row order
Status BooleanSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out) {
  const arrow::Datum v(values.ToArrayData());
  if (values.length == 0) {
    ARROW_ASSIGN_OR_RAISE(out->buffers[1], AllocDevice(8));
    return Status::OK();
  }
  ARROW_ASSIGN_OR_RAISE(arrow::Datum trues, cp::CallFunction("indices_nonzero", {v}, ctx));          // valid and true, ascending rows
  ARROW_ASSIGN_OR_RAISE(arrow::Datum inverted, cp::CallFunction("invert", {v}, ctx));               // (nulls stay null)
  ARROW_ASSIGN_OR_RAISE(arrow::Datum falses, cp::CallFunction("indices_nonzero", {inverted}, ctx));
  ARROW_ASSIGN_OR_RAISE(arrow::Datum is_null, cp::CallFunction("is_null", {v}, ctx));
  ARROW_ASSIGN_OR_RAISE(arrow::Datum nulls, cp::CallFunction("indices_nonzero", {is_null}, ctx));
  std::vector<std::shared_ptr<ArrayData>> parts;
  const bool descending = options.order == cp::SortOrder::Descending;
  if (options.null_placement == cp::NullPlacement::AtStart) parts.push_back(nulls.array());
  parts.push_back(descending ? trues.array() : falses.array());
  parts.push_back(descending ? falses.array() : trues.array());
  if (options.null_placement != cp::NullPlacement::AtStart) parts.push_back(nulls.array());
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ARROW_ASSIGN_OR_RAISE(auto whole, ConcatOnDevice(arrow::uint64(), parts, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  if (whole->length != values.length) return Status::Invalid("arrow_amd: boolean sort lost rows");
  if (whole->offset != 0) return Status::Invalid("arrow_amd: boolean sort: concatenation with an offset");
  out->buffers[1] = whole->buffers[1];
  return Status::OK();
}

// array_sort_indices of a device-resident struct array (declared in plugin/sort.inc, slot 23) — the reference's algorithm
// (ArrayCompareSorter<StructType>, vector_array_sort.cc:266-290): the null structs go to their end in row order
// (PartitionNullsOnly on the struct's own validity), the others are sorted by SortStructArray (vector_sort.cc:1115-1137) =
// a record-batch sort with every field a key, all in the options' order and null placement.  Here: the rows of the valid and
// of the null structs (two GetTakeIndices), the fields gathered at the valid rows (array_take), the multi-key chain above
// over them, and rows[perm] laid before / behind the null rows.  Without a null struct the chain runs over the fields' slices.
Status StructSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out) {
  const std::shared_ptr<ArrayData> data = values.ToArrayData();
  const int64_t n = data->length;
  if (n == 0) {
    ARROW_ASSIGN_OR_RAISE(out->buffers[1], AllocDevice(8));
    return Status::OK();
  }
  if (data->child_data.empty()) return Status::Invalid("Must specify one or more sort keys");
  std::vector<arrow::Datum> columns;
  for (const auto& child : data->child_data) columns.emplace_back(child->Slice(data->offset, n));
  // (an ArraySpan over device buffers reports null_count 0 — Buffer::data() is null off the CPU, ArraySpan::SetMembers —
  //  so the bitmap's presence decides)
  const bool has_nulls = data->buffers[0] != nullptr;
  const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
  arrow::Datum rows, null_rows;
  if (has_nulls) {
    const arrow::Datum is_valid(ArrayData::Make(arrow::boolean(), n, {nullptr, data->buffers[0]}, /*null_count=*/0, data->offset));
    ARROW_ASSIGN_OR_RAISE(rows, cp::CallFunction("indices_nonzero", {is_valid}, ctx));
    ARROW_ASSIGN_OR_RAISE(arrow::Datum inverted, cp::CallFunction("invert", {is_valid}, ctx));
    ARROW_ASSIGN_OR_RAISE(null_rows, cp::CallFunction("indices_nonzero", {inverted}, ctx));
    for (arrow::Datum& c : columns) {
      ARROW_ASSIGN_OR_RAISE(c, cp::CallFunction("array_take", {c, rows}, &no_check, ctx));
    }
  }
  std::vector<DeviceSortKey> keys;
  for (const arrow::Datum& c : columns) keys.push_back(DeviceSortKey{c, options.order, options.null_placement});
  ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, SortIndicesByKeysOnDevice(keys, ctx));
  if (!has_nulls) {
    out->buffers[1] = perm.array()->buffers[1];
    return Status::OK();
  }
  ARROW_ASSIGN_OR_RAISE(arrow::Datum sorted_rows, cp::CallFunction("array_take", {rows, perm}, &no_check, ctx));
  std::vector<std::shared_ptr<ArrayData>> parts;
  if (options.null_placement == cp::NullPlacement::AtStart) parts.push_back(null_rows.array());
  parts.push_back(sorted_rows.array());
  if (options.null_placement != cp::NullPlacement::AtStart) parts.push_back(null_rows.array());
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ARROW_ASSIGN_OR_RAISE(auto whole, ConcatOnDevice(arrow::uint64(), parts, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  if (whole->length != n || whole->offset != 0) return Status::Invalid("arrow_amd: struct sort lost rows");
  out->buffers[1] = whole->buffers[1];
  return Status::OK();
}

// array_sort_indices of a device-resident dictionary array (declared in plugin/sort.inc, slot 20) — the reference's algorithm
// (ArrayCompareSorter<DictionaryType>, vector_array_sort.cc:180-265): 1) dense ascending ranks of the dictionary values, their
// nulls pasted back (RanksWithNulls, :230-262) — on a host copy of the values, through "rank" (host data: the stock function;
// every value type the reference ranks); 2) the ranks decoded through the indices (Take) and 3) sorted as uint64 keys — both on
// the device, where the rows are.
Status DictionarySortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out) {
  const std::shared_ptr<ArrayData> data = values.ToArrayData();
  const int64_t n = data->length;
  if (data->dictionary == nullptr) return Status::Invalid("arrow_amd: a dictionary array without a dictionary");
  if (n == 0) {
    ARROW_ASSIGN_OR_RAISE(out->buffers[1], AllocDevice(8));
    return Status::OK();
  }
  const auto& dict_type = static_cast<const arrow::DictionaryType&>(*data->type);
  ARROW_ASSIGN_OR_RAISE(auto rocm, RocmMemoryManagerFor(0));
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  std::shared_ptr<ArrayData> decoded;
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<ArrayData> dict_host, CopyDataToHost(*data->dictionary));
  const int64_t dict_nulls = dict_host->GetNullCount();
  if (dict_host->length == 0 || dict_nulls == dict_host->length) {
    // (vector_array_sort.cc:207-212: nothing but nulls can come out of the decoding — an all-null uint64 column)
    ARROW_ASSIGN_OR_RAISE(auto zeros, AllocDevice(n * 8));
    ARROW_ASSIGN_OR_RAISE(auto no_bits, AllocDevice(((n + 63) / 64) * 8 + 8));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(no_bits->mutable_address()), 0, static_cast<size_t>(((n + 63) / 64) * 8 + 8), st));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(zeros->mutable_address()), 0, static_cast<size_t>(n * 8), st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    decoded = ArrayData::Make(arrow::uint64(), n, {std::move(no_bits), std::move(zeros)}, n);
  } else {
    std::shared_ptr<Buffer> null_bitmap;
    std::shared_ptr<ArrayData> plain = dict_host;
    if (dict_nulls > 0) {
      ARROW_ASSIGN_OR_RAISE(null_bitmap, arrow::internal::CopyBitmap(ctx->memory_pool(), dict_host->buffers[0]->data(), dict_host->offset,
                                                                     dict_host->length));
      plain = dict_host->Copy();
      plain->buffers[0] = nullptr;
      plain->null_count = 0;
    }
    const cp::RankOptions rank_options(cp::SortOrder::Ascending, cp::RankOptions::Dense);
    ARROW_ASSIGN_OR_RAISE(arrow::Datum rank_datum, cp::CallFunction("rank", {arrow::Datum(plain)}, &rank_options, ctx));
    const auto& rank_data = rank_datum.array();
    ARROW_ASSIGN_OR_RAISE(auto ranks_dev, arrow::MemoryManager::CopyBuffer(rank_data->buffers[1], rocm));
    std::shared_ptr<Buffer> bits_dev;
    if (null_bitmap != nullptr) {
      ARROW_ASSIGN_OR_RAISE(bits_dev, arrow::MemoryManager::CopyBuffer(null_bitmap, rocm));
    }
    auto ranks = ArrayData::Make(arrow::uint64(), rank_data->length, {std::move(bits_dev), std::move(ranks_dev)},
                                 null_bitmap != nullptr ? dict_nulls : 0, rank_data->offset);
    auto indices = ArrayData::Make(dict_type.index_type(), n, {data->buffers[0], data->buffers[1]},
                                   data->buffers[0] == nullptr ? 0 : arrow::kUnknownNullCount, data->offset);
    const cp::TakeOptions take_options = cp::TakeOptions::Defaults();
    ARROW_ASSIGN_OR_RAISE(arrow::Datum taken, cp::CallFunction("array_take", {arrow::Datum(ranks), arrow::Datum(indices)}, &take_options, ctx));
    decoded = taken.array();
  }
  ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, cp::CallFunction("array_sort_indices", {arrow::Datum(decoded)}, &options, ctx));
  if (perm.array()->offset != 0 || !DataOnRocm(*perm.array())) return Status::Invalid("arrow_amd: dictionary sort: unexpected result layout");
  out->buffers[1] = perm.array()->buffers[1];
  return Status::OK();
}

// sort_indices on device-resident record batches, tables and chunked arrays: SortIndicesMetaFunction
// (kernels/vector_sort.cc:850-954) hands those to CPU sorters; the re-registered wrapper resolves the sort keys the
// same way and runs the chain above.  Arrays and host data go to the stock meta-function (whose array path calls
// array_sort_indices by name, i.e. the registered kernel).
class RocmSortIndicesMetaFunction : public cp::MetaFunction {
 public:
  explicit RocmSortIndicesMetaFunction(std::shared_ptr<cp::Function> stock)
      : cp::MetaFunction("sort_indices", cp::Arity::Unary(), stock->doc(), stock->default_options()),
        stock_(std::move(stock)) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args, const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    if (args.size() != 1 || options == nullptr) return stock_->Execute(args, options, ctx);
    const auto& sort_options = *static_cast<const cp::SortOptions*>(options);
    const std::vector<cp::SortKey> sort_keys = sort_options.GetSortKeys();   // (per-key placement, deprecated override applied)
    std::vector<DeviceSortKey> keys;
    // a column in several chunks is concatenated in HBM first (the reference's ChunkedArray sorters number the rows of the
    // logical column, vector_sort.cc:850-954: so do the indices below); decimal128 chunks: as fixed-width 16-byte values
    auto one_chunk = [](const arrow::ChunkedArray& c) -> arrow::Result<arrow::Datum> {
      if (c.num_chunks() == 1) return arrow::Datum(c.chunk(0)->data());
      if (c.num_chunks() == 0) return Status::NotImplemented("arrow_amd: sort_indices of a column without chunks");
      hipStream_t st;
      ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
      std::vector<std::shared_ptr<ArrayData>> chunks;
      for (const auto& chunk : c.chunks()) chunks.push_back(chunk->data());
      ARROW_ASSIGN_OR_RAISE(auto whole, ConcatOnDevice(c.type(), chunks, st));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      return arrow::Datum(whole);
    };
    switch (args[0].kind()) {
      case arrow::Datum::CHUNKED_ARRAY: {
        const auto& c = *args[0].chunked_array();
        bool on_device = false;
        for (const auto& chunk : c.chunks()) on_device = on_device || DataOnRocm(*chunk->data());
        if (!on_device) return stock_->Execute(args, options, ctx);
        if (sort_keys.size() != 1) return Status::Invalid("Must specify exactly one sort key for a chunked array");
        ARROW_ASSIGN_OR_RAISE(auto column, one_chunk(c));
        keys.push_back(DeviceSortKey{column, sort_keys[0].order, sort_keys[0].null_placement});
        break;
      }
      case arrow::Datum::RECORD_BATCH: {
        const auto& batch = *args[0].record_batch();
        bool on_device = false;
        for (int i = 0; i < batch.num_columns(); ++i) on_device = on_device || DataOnRocm(*batch.column_data(i));
        if (!on_device) return stock_->Execute(args, options, ctx);
        for (const auto& sk : sort_keys) {
          ARROW_ASSIGN_OR_RAISE(auto path, sk.target.FindOne(*batch.schema()));
          if (path.indices().size() != 1) return Status::NotImplemented("arrow_amd: nested sort key references");
          keys.push_back(DeviceSortKey{arrow::Datum(batch.column_data(path[0])), sk.order, sk.null_placement});
        }
        break;
      }
      case arrow::Datum::TABLE: {
        const auto& table = *args[0].table();
        bool on_device = false;
        for (int i = 0; i < table.num_columns(); ++i) {
          for (const auto& chunk : table.column(i)->chunks()) on_device = on_device || DataOnRocm(*chunk->data());
        }
        if (!on_device) return stock_->Execute(args, options, ctx);
        for (const auto& sk : sort_keys) {
          ARROW_ASSIGN_OR_RAISE(auto path, sk.target.FindOne(*table.schema()));
          if (path.indices().size() != 1) return Status::NotImplemented("arrow_amd: nested sort key references");
          ARROW_ASSIGN_OR_RAISE(auto column, one_chunk(*table.column(path[0])));
          keys.push_back(DeviceSortKey{column, sk.order, sk.null_placement});
        }
        break;
      }
      default:
        return stock_->Execute(args, options, ctx);
    }
    if (args[0].length() == 0) {
      return arrow::Datum(ArrayData::Make(arrow::uint64(), 0, {nullptr, nullptr}, 0));
    }
    return SortIndicesByKeysOnDevice(keys, ctx);
  }

 private:
  std::shared_ptr<cp::Function> stock_;
};

class RocmOrderByNode : public AccumulatingNode {
 public:
  struct Key {
    int column;
    cp::SortOrder order;
    cp::NullPlacement placement;
  };

  RocmOrderByNode(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs, std::shared_ptr<arrow::Schema> schema,
                  cp::Ordering ordering, std::vector<Key> keys)
      : AccumulatingNode(plan, std::move(inputs), {"input"}, std::move(schema)),
        ordering_(std::move(ordering)), keys_(std::move(keys)) {}

  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                           const ac::ExecNodeOptions& options) {
    if (inputs.size() != 1) return Status::Invalid("order_by_rocm takes exactly one input");
    const auto* opts = dynamic_cast<const ac::OrderByNodeOptions*>(&options);
    if (opts == nullptr) return Status::TypeError("order_by_rocm expects OrderByNodeOptions");
    if (opts->ordering.is_implicit() || opts->ordering.is_unordered()) {
      return Status::Invalid("`ordering` must be an explicit non-empty ordering");      // order_by_node.cc:58-61
    }
    const auto& schema = inputs[0]->output_schema();
    std::vector<Key> keys;
    for (const auto& sk : opts->ordering.sort_keys()) {
      ARROW_ASSIGN_OR_RAISE(auto path, sk.target.FindOne(*schema));
      if (path.indices().size() != 1) return Status::NotImplemented("order_by_rocm: nested field references");
      if (!IsDeviceSortKeyType(*schema->field(path[0])->type())) {
        return Status::NotImplemented("order_by_rocm: sort key of type ", schema->field(path[0])->type()->ToString());
      }
      // (the Ordering-wide placement, deprecated in 25.0.0, overrides the per-key one: api_vector.h:132-143)
      const auto override_placement = opts->ordering.null_placement();
      keys.push_back(Key{path[0], sk.order, override_placement.has_value() ? *override_placement : sk.null_placement});
    }
    for (const auto& f : schema->fields()) {
      const auto& t = *f->type();
      if (FixedByteWidth(t) == 0 && t.id() != Type::BOOL && !IsInt32Binary(t)) {
        return Status::NotImplemented("order_by_rocm: column of type ", t.ToString());
      }
    }
    return plan->EmplaceNode<RocmOrderByNode>(plan, std::move(inputs), schema, opts->ordering, std::move(keys));
  }

  const char* kind_name() const override { return "RocmOrderByNode"; }
  const cp::Ordering& ordering() const override { return ordering_; }

 private:
  Status Finish() override {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    cp::ExecContext* ctx = plan_->query_context()->exec_context();
    // (arrival order is the tie-break in the reference: its queue is filled as batches arrive)
    std::vector<cp::ExecBatch>& batches = batches_[0];
    OrderBatchesByIndex(&batches);
    const int ncols = output_schema_->num_fields();
    int64_t n = 0;
    bool any_device = false;
    for (const auto& b : batches) n += b.length;
    std::vector<arrow::Datum> whole(ncols);
    for (int c = 0; c < ncols; ++c) {
      ARROW_ASSIGN_OR_RAISE(auto col, WholeColumn(batches, output_schema_->field(c)->type(), c, st, &any_device, "order_by_rocm"));
      whole[c] = arrow::Datum(std::move(col));
    }
    batches.clear();
    if (n == 0) return output_->InputFinished(this, 0);
    const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
    std::vector<DeviceSortKey> chain;
    for (const auto& key : keys_) chain.push_back(DeviceSortKey{whole[key.column], key.order, key.placement});
    ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, SortIndicesByKeysOnDevice(chain, ctx));
    std::vector<arrow::Datum> sorted(ncols);
    for (int c = 0; c < ncols; ++c) {
      ARROW_ASSIGN_OR_RAISE(sorted[c], cp::CallFunction("array_take", {whole[c], perm}, &no_check, ctx));
      whole[c] = arrow::Datum();      // (release the concatenated input as we go)
    }
    CountGpu(kFnOrderBy);
    return EmitResult(this, output_, std::move(sorted), n, any_device, st);
  }

  const cp::Ordering ordering_;
  const std::vector<Key> keys_;
};
