// Key rows wider than one Grouper table: the key columns, the rule that spreads them over a chain of tables, the chain.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// Users: aggregate_rocm's general node (plugin/acero_node_general.inc) and hashjoin_rocm (plugin/hash_join_node.inc).

// a Grouper key column: the span the table reads, its bytes per row and the buffers that keep it alive
struct KeyColumn {
  ArxSpan span;
  int32_t width;
  bool joined_to_next = false;   // this column and the next one go into the same table (the halves of a string chunk)
  std::vector<std::shared_ptr<Buffer>> keep;
};

// One device table holds rows of up to 16 bytes / 8 columns (32-byte slots, csrc/grouper.hip); wider rows go through a
// CHAIN of tables instead of wider slots: level 0 maps the first columns to ids, level s maps (id of level s - 1, the next
// columns).  A 4-byte id stands for everything to its left, and a row's tuple (prefix id, columns) appears first exactly
// where the row does, so the last level's ids are the ids of the whole row in order of first appearance (the reference
// encodes the whole row, row/grouper.cc:559-611).  Returns the positions into `cols` that each level takes.  This is the
// only statement of the rule on the C++ side; the mirror states the same rule in compute.py::_grouper_levels (without
// the pairing: where a level ends changes no id, only which table holds a column).
std::vector<std::vector<int>> PlanGrouperLevels(const std::vector<KeyColumn>& cols) {
  std::vector<std::vector<int>> levels(1);
  int used = 0;
  for (int j = 0; j < static_cast<int>(cols.size()); ++j) {
    const bool later = levels.size() > 1;
    const bool pair = cols[j].joined_to_next && j + 1 < static_cast<int>(cols.size());
    const int need = cols[j].width + (pair ? cols[j + 1].width : 0);
    if (!levels.back().empty() && (used + need > 16 || static_cast<int>(levels.back().size()) + (later ? 1 : 0) + (pair ? 2 : 1) > 8)) {
      levels.emplace_back();
      used = 4;
    }
    levels.back().push_back(j);
    used += cols[j].width;
  }
  return levels;
}

// A utf8 / binary key is, for the Grouper, its length (uint32, 0xFFFFFFFF = null) followed by 12 bytes of the string per
// chunk as a uint64 and a uint32 column (arx_binary_key_lengths / _chunk): equal strings agree in all of them, different
// strings differ in the length or in some chunk.  BinaryKeyLengths makes the length column and reports the longest
// string; BinaryKeyColumns appends that column and the chunks that strings of up to `max_len_for_chunks` bytes need
// (a join passes the larger of its two sides' lengths: the shorter side's extra chunks are zero).
arrow::Result<KeyColumn> BinaryKeyLengths(const ArxBinarySpan& bs, int64_t n, hipStream_t st, int64_t* max_len) {
  ARROW_ASSIGN_OR_RAISE(auto lens, AllocDevice(std::max<int64_t>(n, 1) * 4));
  *max_len = 0;
  if (n > 0) {
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &ws));
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_key_lengths(&bs, DevPtr<uint32_t>(lens), max_len, ws, st)));
  }
  return KeyColumn{ArxSpan{nullptr, DevPtr<void>(lens), 0, n, 0}, 4, false, {lens}};
}

Status BinaryKeyColumns(const ArxBinarySpan& bs, int64_t n, KeyColumn lengths, int64_t max_len_for_chunks, hipStream_t st,
                        std::vector<KeyColumn>* out) {
  out->push_back(std::move(lengths));
  for (int64_t c = 0; c * 12 < max_len_for_chunks; ++c) {
    ARROW_ASSIGN_OR_RAISE(auto lo, AllocDevice(std::max<int64_t>(n, 1) * 8));
    ARROW_ASSIGN_OR_RAISE(auto hi, AllocDevice(std::max<int64_t>(n, 1) * 4));
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_key_chunk(&bs, c, DevPtr<uint64_t>(lo), DevPtr<uint32_t>(hi), st)));
    out->push_back(KeyColumn{ArxSpan{nullptr, DevPtr<void>(lo), 0, n, 0}, 8, true, {lo}});
    out->push_back(KeyColumn{ArxSpan{nullptr, DevPtr<void>(hi), 0, n, 0}, 4, false, {hi}});
  }
  return Status::OK();
}

// The chain of Grouper tables (compute.Grouper), one table per level, kept so that rows can be looked up after others were
// consumed.  consume: ids, never null; lookup: ids and their validity (an unseen prefix is a null id, which no consumed
// row has).
struct GrouperChain {
  std::vector<std::vector<int>> levels;
  std::vector<AlignedDevice> states;
  int64_t max_groups = 1;
  int64_t num_groups = 0;   // of the whole row, after a consume

  static arrow::Result<GrouperChain> Make(std::vector<std::vector<int>> levels, int64_t max_groups, hipStream_t st) {
    GrouperChain chain;
    chain.levels = std::move(levels);
    chain.max_groups = std::max<int64_t>(max_groups, 1);
    for (size_t s = 0; s < chain.levels.size(); ++s) {
      ARROW_ASSIGN_OR_RAISE(auto state, AllocAligned(static_cast<int64_t>(arx_grouper_state_bytes(chain.max_groups))));
      ARROW_RETURN_NOT_OK(FromArx(arx_grouper_init(state.ptr, chain.max_groups, st)));
      chain.states.push_back(std::move(state));
    }
    return chain;
  }

  Status Run(const std::vector<KeyColumn>& cols, int64_t n, bool lookup, hipStream_t st, std::shared_ptr<Buffer>* out_ids,
             std::shared_ptr<Buffer>* out_valid) {
    std::shared_ptr<Buffer> ids, valid;
    const size_t ws_bytes = arx_grouper_consume_workspace_bytes(n);
    ARROW_ASSIGN_OR_RAISE(auto ws, AllocAligned(static_cast<int64_t>(ws_bytes)));
    for (size_t s = 0; s < levels.size(); ++s) {
      std::vector<ArxSpan> spans;
      std::vector<int32_t> widths;
      if (s > 0) {
        spans.push_back(ArxSpan{DevPtr<void>(valid), DevPtr<void>(ids), 0, n, valid != nullptr ? arrow::kUnknownNullCount : 0});
        widths.push_back(4);
      }
      for (int j : levels[s]) {
        spans.push_back(cols[j].span);
        widths.push_back(cols[j].width);
      }
      ARROW_ASSIGN_OR_RAISE(auto next_ids, AllocDevice(std::max<int64_t>(n, 1) * 4));
      void* state = states[s].ptr;
      if (lookup) {
        ARROW_ASSIGN_OR_RAISE(auto next_valid, ZeroedDevice(BitmapBytes(n), st));
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_lookup(state, max_groups, spans.data(), widths.data(), static_cast<int>(spans.size()), ws.ptr,
                                                       ws_bytes, DevPtr<uint32_t>(next_ids), DevPtr<uint8_t>(next_valid), st)));
        valid = std::move(next_valid);
      } else {
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_consume(state, max_groups, spans.data(), widths.data(), static_cast<int>(spans.size()), ws.ptr,
                                                        ws_bytes, DevPtr<uint32_t>(next_ids), st)));
      }
      ids = std::move(next_ids);
      if (!lookup && s + 1 == levels.size()) {
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_num_groups(state, &num_groups, st)));
      }
    }
    *out_ids = std::move(ids);
    if (out_valid != nullptr) *out_valid = std::move(valid);
    return Status::OK();
  }
};
