// What the Acero exec nodes share: the accumulate-then-finish protocol, batch order, whole columns, the result's way out.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
namespace ac = arrow::acero;

// ---------------------------------------------------------------- small helpers
// a validity (or boolean value) bitmap of `rows` bits in whole 64-bit words, plus the word the kernels may read past
int64_t BitmapBytes(int64_t rows) { return ((rows + 63) / 64) * 8 + 8; }

// Tables and workspaces of the arx_* operators start on 256-byte boundaries: ask for 256 bytes more, round the address up.
void* Align256(void* p) { return reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(p) + 255) & ~uintptr_t(255)); }
struct AlignedDevice {
  std::shared_ptr<Buffer> buffer;   // keeps `ptr` alive
  void* ptr;
};
arrow::Result<AlignedDevice> AllocAligned(int64_t bytes) {
  ARROW_ASSIGN_OR_RAISE(auto buffer, AllocDevice(bytes + 256));
  void* ptr = Align256(reinterpret_cast<void*>(buffer->mutable_address()));
  return AlignedDevice{std::move(buffer), ptr};
}

template <typename T>
T* DevPtr(const std::shared_ptr<Buffer>& b) { return b == nullptr ? nullptr : reinterpret_cast<T*>(b->mutable_address()); }

arrow::Result<std::shared_ptr<Buffer>> ZeroedDevice(int64_t bytes, hipStream_t st) {
  ARROW_ASSIGN_OR_RAISE(auto buf, AllocDevice(std::max<int64_t>(bytes, 8)));
  HIP_RETURN_NOT_OK(hipMemsetAsync(DevPtr<void>(buf), 0, static_cast<size_t>(std::max<int64_t>(bytes, 8)), st));
  return buf;
}

// array data, children and dictionary included, copied to host memory (dictionaries: small by nature)
arrow::Result<std::shared_ptr<ArrayData>> CopyDataToHost(const ArrayData& d) {
  std::vector<std::shared_ptr<Buffer>> bufs(d.buffers.size());
  for (size_t i = 0; i < bufs.size(); ++i) {
    if (d.buffers[i] == nullptr) continue;
    if (d.buffers[i]->is_cpu()) {
      bufs[i] = d.buffers[i];
    } else {
      ARROW_ASSIGN_OR_RAISE(bufs[i], arrow::MemoryManager::CopyBuffer(d.buffers[i], arrow::default_cpu_memory_manager()));
    }
  }
  // (a device array's null count is not to be trusted when a validity buffer exists: see DeviceSpan)
  auto host = ArrayData::Make(d.type, d.length, std::move(bufs), bufs.empty() || d.buffers[0] == nullptr ? 0 : arrow::kUnknownNullCount, d.offset);
  for (const auto& child : d.child_data) {
    ARROW_ASSIGN_OR_RAISE(auto hc, CopyDataToHost(*child));
    host->child_data.push_back(std::move(hc));
  }
  if (d.dictionary != nullptr) {
    ARROW_ASSIGN_OR_RAISE(host->dictionary, CopyDataToHost(*d.dictionary));
  }
  return host;
}

// ---------------------------------------------------------------- Concatenate on the device
const uint8_t* DeviceBytes(const std::shared_ptr<Buffer>& b) {
  return b ? reinterpret_cast<const uint8_t*>(b->address()) : nullptr;
}

// bits [offset, offset+length) of a host or device bitmap (nullptr = all ones) appended at `dst_bit`
Status AppendBits(const std::shared_ptr<Buffer>& src, bool on_device, int64_t offset, int64_t length,
                         uint8_t* dst, int64_t dst_bit, hipStream_t st) {
  if (length == 0) return Status::OK();
  const void* bits = nullptr;
  int64_t bit_offset = offset;
  if (src != nullptr && !on_device) {
    const int64_t first = offset / 8, last = (offset + length + 7) / 8;
    void* staged = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kValidity, static_cast<size_t>(last - first) + 16, &staged));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(staged, src->data() + first, last - first, hipMemcpyHostToDevice, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (pageable source; the slot is reused by the next chunk)
    bits = staged;
    bit_offset = offset % 8;
  } else if (src != nullptr) {
    bits = DeviceBytes(src);
  }
  return FromArx(arx_bitmap_copy_at(bits, bit_offset, length, dst, dst_bit, st));
}

// Concatenate (array/concatenate.cc) of one column's chunks into one device-resident array
arrow::Result<std::shared_ptr<ArrayData>> ConcatOnDevice(const std::shared_ptr<arrow::DataType>& type,
                                                                const std::vector<std::shared_ptr<ArrayData>>& chunks,
                                                                hipStream_t st) {
  int64_t n = 0;
  bool any_validity = false;
  for (const auto& c : chunks) {
    n += c->length;
    any_validity = any_validity || (c->buffers[0] != nullptr && c->null_count.load() != 0);
  }
  // consecutive slices of one device array (what table_source cuts a device table into): nothing to copy
  bool contiguous = !chunks.empty() && DataOnRocm(*chunks[0]);
  for (size_t i = 1; contiguous && i < chunks.size(); ++i) {
    const auto &a = *chunks[i - 1], &b = *chunks[i];
    contiguous = a.buffers.size() == b.buffers.size() && a.offset + a.length == b.offset;
    for (size_t j = 0; contiguous && j < a.buffers.size(); ++j) contiguous = a.buffers[j] == b.buffers[j];
  }
  if (contiguous) {
    const auto& first = *chunks[0];
    int64_t null_count = 0;
    if (first.buffers[0] != nullptr) {
      void* ws = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &ws));
      int64_t set_bits = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_popcount(DeviceBytes(first.buffers[0]), first.offset, n, ws, 64, &set_bits, st)));
      null_count = n - set_bits;
    }
    return ArrayData::Make(type, n, first.buffers, null_count, first.offset);
  }
  const int64_t bitmap_bytes = ((n + 63) / 64) * 8;
  std::shared_ptr<Buffer> validity;
  if (any_validity) {
    ARROW_ASSIGN_OR_RAISE(validity, AllocDevice(bitmap_bytes));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(validity->mutable_address()), 0, bitmap_bytes, st));
    int64_t pos = 0;
    for (const auto& c : chunks) {
      const bool has = c->buffers[0] != nullptr && c->null_count.load() != 0;
      ARROW_RETURN_NOT_OK(AppendBits(has ? c->buffers[0] : nullptr, DataOnRocm(*c), c->offset, c->length,
                                     reinterpret_cast<uint8_t*>(validity->mutable_address()), pos, st));
      pos += c->length;
    }
  }
  std::vector<std::shared_ptr<Buffer>> bufs{validity};
  if (type->id() == Type::BOOL) {
    ARROW_ASSIGN_OR_RAISE(auto data, AllocDevice(bitmap_bytes));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(data->mutable_address()), 0, bitmap_bytes, st));
    int64_t pos = 0;
    for (const auto& c : chunks) {
      ARROW_RETURN_NOT_OK(AppendBits(c->buffers[1], DataOnRocm(*c), c->offset, c->length,
                                     reinterpret_cast<uint8_t*>(data->mutable_address()), pos, st));
      pos += c->length;
    }
    bufs.push_back(std::move(data));
  } else if (IsInt32Binary(*type)) {
    // where each chunk's bytes start and end (two offsets per chunk; read back for device chunks)
    std::vector<std::pair<int32_t, int32_t>> range(chunks.size(), {0, 0});
    int64_t total = 0;
    for (size_t i = 0; i < chunks.size(); ++i) {
      const auto& c = *chunks[i];
      if (c.length == 0) continue;
      if (DataOnRocm(c)) {
        const uint8_t* off = DeviceBytes(c.buffers[1]);
        HIP_RETURN_NOT_OK(hipMemcpyAsync(&range[i].first, off + c.offset * 4, 4, hipMemcpyDeviceToHost, st));
        HIP_RETURN_NOT_OK(hipMemcpyAsync(&range[i].second, off + (c.offset + c.length) * 4, 4, hipMemcpyDeviceToHost, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      } else {
        const int32_t* off = reinterpret_cast<const int32_t*>(c.buffers[1]->data());
        range[i] = {off[c.offset], off[c.offset + c.length]};
      }
      total += range[i].second - range[i].first;
    }
    if (total > INT32_MAX) return Status::Invalid("offset overflow while concatenating arrays");   // concatenate.cc PutOffsets
    ARROW_ASSIGN_OR_RAISE(auto offsets, AllocDevice((n + 1) * 4));
    ARROW_ASSIGN_OR_RAISE(auto data, AllocDevice(total));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(offsets->mutable_address()), 0, (n + 1) * 4, st));
    int64_t pos = 0;
    int32_t base = 0;
    for (size_t i = 0; i < chunks.size(); ++i) {
      const auto& c = *chunks[i];
      if (c.length == 0) continue;
      const bool dev = DataOnRocm(c);
      const int32_t* src_off = nullptr;
      if (dev) {
        src_off = reinterpret_cast<const int32_t*>(DeviceBytes(c.buffers[1])) + c.offset;
      } else {
        void* staged = nullptr;
        ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(c.length + 1) * 4, &staged));
        HIP_RETURN_NOT_OK(hipMemcpyAsync(staged, c.buffers[1]->data() + c.offset * 4, (c.length + 1) * 4,
                                         hipMemcpyHostToDevice, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
        src_off = static_cast<const int32_t*>(staged);
      }
      ARROW_RETURN_NOT_OK(FromArx(arx_binary_rebase_offsets(
          src_off, c.length, base, reinterpret_cast<int32_t*>(offsets->mutable_address()) + pos, st)));
      const int64_t nbytes = range[i].second - range[i].first;
      if (nbytes > 0) {
        const uint8_t* src = (dev ? DeviceBytes(c.buffers[2]) : c.buffers[2]->data()) + range[i].first;
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(data->mutable_address()) + base, src, nbytes,
                                         dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (!dev) HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      }
      pos += c.length;
      base += static_cast<int32_t>(nbytes);
    }
    bufs.push_back(std::move(offsets));
    bufs.push_back(std::move(data));
  } else {
    const int w = FixedByteWidth(*type);
    ARROW_ASSIGN_OR_RAISE(auto data, AllocDevice(n * w));
    int64_t pos = 0;
    for (const auto& c : chunks) {
      if (c->length == 0) continue;
      const bool dev = DataOnRocm(*c);
      const uint8_t* src = (dev ? DeviceBytes(c->buffers[1]) : c->buffers[1]->data()) + c->offset * w;
      HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(data->mutable_address()) + pos * w, src,
                                       c->length * w, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
      if (!dev) HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      pos += c->length;
    }
    bufs.push_back(std::move(data));
  }
  int64_t null_count = 0;
  if (any_validity) {
    ARROW_ASSIGN_OR_RAISE(null_count, DeviceNullCount(*validity, n, st));   // exact: nothing may popcount it on the CPU
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  return ArrayData::Make(type, n, std::move(bufs), null_count, 0);
}

// ---------------------------------------------------------------- the accumulate-then-finish protocol
// A pipeline breaker over one or two inputs.  Acero may deliver batches from any thread and in any order, and
// InputFinished (the input's batch count) may arrive before the last batch: an AtomicCounter per input says when that
// input is complete, whichever call completes it.  Batches are handed to Accept under the node's mutex (the default
// keeps them in batches_[input]); when the last input completes, Finish runs once, under the same mutex, on the thread
// that completed it.  Nothing is produced before that, so there is nothing to start, pause, resume or stop.
class AccumulatingNode : public ac::ExecNode {
 public:
  using ac::ExecNode::ExecNode;

  Status InputReceived(ac::ExecNode* input, cp::ExecBatch batch) override {
    const int i = input == inputs_[0] ? 0 : 1;
    {
      std::lock_guard<std::mutex> lock(mu_);
      ARROW_RETURN_NOT_OK(Accept(i, std::move(batch)));
    }
    return counter_[i].Increment() ? InputDone() : Status::OK();
  }
  Status InputFinished(ac::ExecNode* input, int total_batches) override {
    return counter_[input == inputs_[0] ? 0 : 1].SetTotal(total_batches) ? InputDone() : Status::OK();
  }
  Status StartProducing() override { return Status::OK(); }
  void PauseProducing(ac::ExecNode*, int32_t) override {}
  void ResumeProducing(ac::ExecNode*, int32_t) override {}

 protected:
  Status StopProducingImpl() override { return Status::OK(); }
  virtual Status Accept(int input, cp::ExecBatch batch) {
    batches_[input].push_back(std::move(batch));
    return Status::OK();
  }
  virtual Status Finish() = 0;

  std::vector<cp::ExecBatch> batches_[2];

 private:
  Status InputDone() {
    if (inputs_done_.fetch_add(1) + 1 < static_cast<int>(inputs_.size())) return Status::OK();
    std::lock_guard<std::mutex> lock(mu_);
    return Finish();
  }

  std::mutex mu_;
  ac::AtomicCounter counter_[2];
  std::atomic<int> inputs_done_{0};
};

// Arrival order depends on the thread schedule; with batch indices present (an ordered source) the batches are put in
// that order, so that row order, and everything that follows from it, does not.  Returns whether every batch had one.
bool OrderBatchesByIndex(std::vector<cp::ExecBatch>* batches) {
  const bool indexed = std::all_of(batches->begin(), batches->end(), [](const cp::ExecBatch& b) { return b.index >= 0; });
  if (indexed) {
    std::stable_sort(batches->begin(), batches->end(), [](const cp::ExecBatch& a, const cp::ExecBatch& b) { return a.index < b.index; });
  }
  return indexed;
}

// one column of all batches as one device array (host chunks are uploaded; an input without rows: an empty device array);
// `node` names the caller in the Status for a scalar column
arrow::Result<std::shared_ptr<ArrayData>> WholeColumn(const std::vector<cp::ExecBatch>& batches, const std::shared_ptr<arrow::DataType>& type,
                                                      int column, hipStream_t st, bool* any_device, const char* node) {
  std::vector<std::shared_ptr<ArrayData>> chunks;
  for (const auto& b : batches) {
    if (!b[column].is_array()) return Status::NotImplemented(node, ": scalar columns");
    if (b.length == 0) continue;
    chunks.push_back(b[column].array());
    *any_device = *any_device || DataOnRocm(*b[column].array());
  }
  if (chunks.empty()) {
    ARROW_ASSIGN_OR_RAISE(auto data, ZeroedDevice(8, st));
    std::vector<std::shared_ptr<Buffer>> bufs{nullptr, data};
    if (IsInt32Binary(*type)) bufs.push_back(data);
    return ArrayData::Make(type, 0, std::move(bufs), 0);
  }
  return ConcatOnDevice(type, chunks, st);
}

// The node's result leaves as batches of `batch_size` rows, numbered from 0, then InputFinished; no rows: no batch.
// any_device == false ("host in, host out"): columns that lie in HBM are copied back first.  A slice of a device array
// must carry its exact null count: whoever asks for it later (Table::FromRecordBatches, ChunkedArray's constructor) would
// otherwise popcount HBM from the CPU, so every unknown count is settled here by arx_bitmap_popcount.
Status EmitResult(ac::ExecNode* self, ac::ExecNode* output, std::vector<arrow::Datum> columns, int64_t rows, bool any_device,
                  hipStream_t st, int64_t batch_size = ac::ExecPlan::kMaxBatchSize) {
  if (rows == 0) return output->InputFinished(self, 0);
  for (auto& column : columns) {
    if (any_device || !DataOnRocm(*column.array())) continue;
    ARROW_ASSIGN_OR_RAISE(auto host, CopyDataToHost(*column.array()));
    column = arrow::Datum(std::move(host));
  }
  const cp::ExecBatch out(std::move(columns), rows);
  const int num_batches = static_cast<int>((rows + batch_size - 1) / batch_size);
  for (int i = 0; i < num_batches; ++i) {
    cp::ExecBatch slice = out.Slice(i * batch_size, batch_size);
    slice.index = i;
    for (auto& value : slice.values) {
      ArrayData* a = value.mutable_array();
      if (!any_device || a->null_count.load() != arrow::kUnknownNullCount || a->buffers[0] == nullptr) continue;
      void* ws = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &ws));
      int64_t set_bits = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_popcount(DeviceBytes(a->buffers[0]), a->offset, a->length, ws, 64, &set_bits, st)));
      a->null_count = a->length - set_bits;
    }
    ARROW_RETURN_NOT_OK(output->InputReceived(self, std::move(slice)));
  }
  return output->InputFinished(self, num_batches);
}
