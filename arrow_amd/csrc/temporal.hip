// Date / time field extraction on gfx950: year, quarter, month, day, day_of_week, day_of_year, iso_year, iso_week of
// date32 / date64 / timestamp[s, ms, us, ns], and hour, minute, second, millisecond, microsecond, nanosecond of
// timestamp[*] / time32[s, ms] / time64[us, ns] — what GROUP BY year(d), WHERE month(ts) = 12 and hour buckets lower to.
//
// What it restates (semantics only):
//   Year / Month / ... / ISOWeek / Hour / ... / Nanosecond   cpp/src/arrow/compute/kernels/scalar_temporal_unary.cc
//   civil_from_days, weekday, iso_week                        cpp/src/arrow/vendored/datetime/date.h
// Proleptic Gregorian calendar, every division a floor division (instants before the epoch are right), int64 results,
// the result's validity = the input's re-based to offset 0, a null result slot written as zero.  No time zones.
//
// Shape: one 64-bit floor division per row at most — to (days, rest of the day) for date64 / timestamp[s, ms, us] and
// time64[us], to (seconds, nanoseconds) for the two nanosecond types, whose seconds then split in 32 bits — by a
// compile-time divisor (a multiply-high: the kernel is templated on the input type); date32 and time32 never leave 32
// bits.  Days are taken as int32: the day count of every instant of years -32767 .. 32767 fits, one that does not wraps
// (the result then depends on the row's value alone, like the reference's own wrapped results out there).  Everything
// after the split is unsigned 32-bit arithmetic on values shifted to be non-negative, so floor and truncation agree.
// A second template parameter picks the decomposition group (civil date, ISO week, weekday, time of day); the component
// inside a group is a wave-uniform switch.
// Memory: a lane takes two consecutive rows (one 16-byte store, one 16- or 8-byte load at whatever alignment the input's
// offset leaves), a wave 128 rows = two validity words (wave-uniform loads) a step and kTemporalSteps steps at a time,
// all loads issued before the first result; the lane whose rows straddle `length` goes row by row.  Plain loads and
// stores: the non-temporal forms were slower here.  A null row enters the arithmetic as 0, never as the
// bytes under it.
#include "arx_common.h"

#include <algorithm>

namespace arx {

// rows one wave takes at a time (tests/test_temporal.py: ROWS_PER_WAVE): 64 lanes x 2 rows x kTemporalSteps
constexpr int kTemporalSteps = 4;
constexpr int64_t kTemporalMaxBlocks = 1 << 20;   // workgroups of a launch (a wave strides over what is left)

enum { kGroupCivil = 0, kGroupIso = 1, kGroupWeekday = 2, kGroupTime = 3 };

static std::atomic<int64_t> g_temporal_civil_launches{0};     // year, quarter, month, day, day_of_year
static std::atomic<int64_t> g_temporal_iso_launches{0};       // iso_year, iso_week
static std::atomic<int64_t> g_temporal_weekday_launches{0};   // day_of_week
static std::atomic<int64_t> g_temporal_time_launches{0};      // hour .. nanosecond
static constexpr CounterRow kTemporalCounters[] = {
    {"temporal_civil_launches", &g_temporal_civil_launches},
    {"temporal_iso_launches", &g_temporal_iso_launches},
    {"temporal_weekday_launches", &g_temporal_weekday_launches},
    {"temporal_time_launches", &g_temporal_time_launches},
};
CounterTable temporal_counters() { return counter_table(kTemporalCounters); }

// ---------------------------------------------------------------- floor division by a constant, without signed division
// v + 2^31 (or 2^63) is non-negative: divide that and take the bias back out of quotient and remainder.
template <uint32_t D>
__device__ __forceinline__ uint32_t floor_mod_i32(int32_t v) {   // v mod D in [0, D)
  constexpr uint32_t kR0 = 0x80000000u % D;
  const uint32_t r = ((static_cast<uint32_t>(v) ^ 0x80000000u) % D) + (D - kR0);
  return r >= D ? r - D : r;
}
template <uint32_t D>
__device__ __forceinline__ int32_t floor_div_i32(int32_t v) {
  constexpr uint32_t kQ0 = 0x80000000u / D, kR0 = 0x80000000u % D;
  const uint32_t u = static_cast<uint32_t>(v) ^ 0x80000000u;
  const uint32_t q = u / D;
  return static_cast<int32_t>(q - kQ0) - ((u - q * D) < kR0 ? 1 : 0);
}
template <uint64_t D>
__device__ __forceinline__ void floor_divmod_i64(int64_t v, int64_t* quotient, uint64_t* remainder) {
  constexpr uint64_t kQ0 = 0x8000000000000000ull / D, kR0 = 0x8000000000000000ull % D;
  const uint64_t u = static_cast<uint64_t>(v) ^ 0x8000000000000000ull;
  const uint64_t q = u / D;
  const uint64_t r = u - q * D;
  const bool borrow = r < kR0;
  *quotient = static_cast<int64_t>(q - kQ0) - (borrow ? 1 : 0);
  *remainder = borrow ? r + (D - kR0) : r - kR0;
}

// ---------------------------------------------------------------- one row, taken apart
struct TemporalParts {
  int32_t days;   // since 1970-01-01 (wrapped to 32 bits)
  uint32_t sod;   // second of the day, 0 .. 86399
  uint32_t sub;   // the rest of the second in the input's unit: 0 (seconds), 0 .. 999 (ms), .. 999999 (us), .. 999999999 (ns)
};

template <int kType>
struct TemporalValue {   // the input's physical type
  using type = int64_t;
};
template <> struct TemporalValue<ARX_TIME_DATE32> { using type = int32_t; };
template <> struct TemporalValue<ARX_TIME_TIME32_S> { using type = int32_t; };
template <> struct TemporalValue<ARX_TIME_TIME32_MS> { using type = int32_t; };

// (what a caller does not use of the result is dead code to the compiler: the civil group never computes `sub`)
template <int kType>
__device__ __forceinline__ TemporalParts temporal_split(typename TemporalValue<kType>::type v) {
  TemporalParts p{0, 0, 0};
  if constexpr (kType == ARX_TIME_DATE32) {
    p.days = v;
  } else if constexpr (kType == ARX_TIME_TIME32_S) {
    p.sod = floor_mod_i32<86400u>(v);
  } else if constexpr (kType == ARX_TIME_TIME32_MS) {
    const uint32_t ms = floor_mod_i32<86400000u>(v);
    p.sod = ms / 1000u;
    p.sub = ms - p.sod * 1000u;
  } else if constexpr (kType == ARX_TIME_TIMESTAMP_NS || kType == ARX_TIME_TIME64_NS) {
    // |seconds| < 2^34: seconds / 86400 = (seconds >> 7) / 675 in 32 bits
    int64_t seconds;
    uint64_t ns;
    floor_divmod_i64<1000000000ull>(v, &seconds, &ns);
    p.sub = static_cast<uint32_t>(ns);
    p.days = floor_div_i32<675u>(static_cast<int32_t>(seconds >> 7));
    p.sod = static_cast<uint32_t>(seconds) - static_cast<uint32_t>(p.days) * 86400u;
  } else {
    constexpr uint64_t kPerSecond = kType == ARX_TIME_TIMESTAMP_S ? 1ull
                                    : (kType == ARX_TIME_TIMESTAMP_US || kType == ARX_TIME_TIME64_US) ? 1000000ull
                                                                                                     : 1000ull;   // date64: ms
    int64_t days;
    uint64_t rest;   // of the day, < 86400 * kPerSecond <= 8.64e10
    floor_divmod_i64<86400ull * kPerSecond>(v, &days, &rest);
    p.days = static_cast<int32_t>(static_cast<uint32_t>(static_cast<uint64_t>(days)));
    if constexpr (kPerSecond == 1ull) {
      p.sod = static_cast<uint32_t>(rest);
    } else if constexpr (kPerSecond == 1000ull) {
      p.sod = static_cast<uint32_t>(rest) / 1000u;
      p.sub = static_cast<uint32_t>(rest) - p.sod * 1000u;
    } else {   // 10^6 = 2^6 x 15625, and rest >> 6 < 2^31
      p.sod = static_cast<uint32_t>(rest >> 6) / 15625u;
      p.sub = static_cast<uint32_t>(rest) - p.sod * 1000000u;   // (modulo 2^32: the true difference is below 10^6)
    }
  }
  return p;
}

// ---------------------------------------------------------------- the calendar, from days
struct Civil {
  int32_t year;
  uint32_t month, day;   // 1 .. 12, 1 .. 31
  uint32_t yday;         // day of the year, 1 .. 366
};

// civil_from_days (date.h) in unsigned arithmetic: the day count is shifted by kEras 400-year eras, which makes it
// non-negative for every day from -2147468786 on — all of the years -32767 .. 32767 and far beyond.  The lowest 14862
// values of int32 wrap around 2^32 instead (no shift avoids that: the span of int32 is 2^32); like every out-of-range
// row they give a value that depends on the row alone.
__device__ __forceinline__ Civil civil_from_days(int32_t days) {
  constexpr uint32_t kEras = 14694;
  const uint32_t z = static_cast<uint32_t>(days) + 719468u + 146097u * kEras;
  const uint32_t era = z / 146097u;
  const uint32_t doe = z - era * 146097u;                                                        // 0 .. 146096
  const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - (doe == 146096u ? 1u : 0u)) / 365u;   // 0 .. 399
  const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                               // 0 .. 365, from 1 March
  const uint32_t mp = (5u * doy + 2u) / 153u;                                                    // 0 .. 11
  const bool jan_feb = mp >= 10u;
  Civil c;
  c.day = doy - (153u * mp + 2u) / 5u + 1u;
  c.month = jan_feb ? mp - 9u : mp + 3u;
  c.year = static_cast<int32_t>(yoe + era * 400u) - static_cast<int32_t>(kEras * 400u) + (jan_feb ? 1 : 0);
  // March .. December lie in the year the era's year-of-era names: it is a leap year by yoe alone (eras start on a year = 0 mod 400)
  const uint32_t leap = ((yoe & 3u) == 0u && (yoe % 100u != 0u || yoe == 0u)) ? 1u : 0u;
  c.yday = jan_feb ? doy - 305u : doy + 60u + leap;
  return c;
}

// Monday = 0 .. Sunday = 6 (1970-01-01 was a Thursday)
__device__ __forceinline__ uint32_t weekday_from_days(int32_t days) { return floor_mod_i32<7u>(static_cast<int32_t>(static_cast<uint32_t>(days) + 3u)); }

template <int kType, int kGroup>
__device__ __forceinline__ int64_t temporal_field(typename TemporalValue<kType>::type v, int component, uint32_t week_start,
                                                  uint32_t count_from_one) {
  const TemporalParts p = temporal_split<kType>(v);
  if constexpr (kGroup == kGroupCivil) {
    const Civil c = civil_from_days(p.days);
    switch (component) {
      case ARX_TEMPORAL_YEAR: return c.year;
      case ARX_TEMPORAL_QUARTER: return (c.month - 1u) / 3u + 1u;
      case ARX_TEMPORAL_MONTH: return c.month;
      case ARX_TEMPORAL_DAY: return c.day;
      default: return c.yday;
    }
  } else if constexpr (kGroup == kGroupIso) {
    // the week's Thursday names the ISO year; its day of the year counts the weeks
    const uint32_t wd = weekday_from_days(p.days);
    const Civil c = civil_from_days(static_cast<int32_t>(static_cast<uint32_t>(p.days) - wd + 3u));
    return component == ARX_TEMPORAL_ISO_YEAR ? static_cast<int64_t>(c.year) : static_cast<int64_t>((c.yday - 1u) / 7u + 1u);
  } else if constexpr (kGroup == kGroupWeekday) {
    const uint32_t d = weekday_from_days(p.days) + 8u - week_start;   // (ISO weekday - week_start + 7): 1 .. 13
    return (d >= 7u ? d - 7u : d) + count_from_one;
  } else {
    constexpr bool kMilli = kType == ARX_TIME_TIMESTAMP_MS || kType == ARX_TIME_TIME32_MS;
    constexpr bool kMicro = kType == ARX_TIME_TIMESTAMP_US || kType == ARX_TIME_TIME64_US;
    constexpr bool kNano = kType == ARX_TIME_TIMESTAMP_NS || kType == ARX_TIME_TIME64_NS;
    switch (component) {
      case ARX_TEMPORAL_HOUR: return p.sod / 3600u;
      case ARX_TEMPORAL_MINUTE: return (p.sod / 60u) % 60u;
      case ARX_TEMPORAL_SECOND: return p.sod % 60u;
      case ARX_TEMPORAL_MILLISECOND: return kMilli ? p.sub : kMicro ? p.sub / 1000u : kNano ? p.sub / 1000000u : 0u;
      case ARX_TEMPORAL_MICROSECOND: return kMicro ? p.sub % 1000u : kNano ? (p.sub / 1000u) % 1000u : 0u;
      default: return kNano ? p.sub % 1000u : 0u;
    }
  }
}

struct I64x2 {
  int64_t a, b;
};

template <int kType, int kGroup>
__global__ __launch_bounds__(kBlock) void temporal_kernel(const typename TemporalValue<kType>::type* __restrict__ in, Bits valid, int64_t n,
                                                          int component, uint32_t week_start, uint32_t count_from_one,
                                                          int64_t* __restrict__ out, uint64_t* __restrict__ out_valid) {
  using T = typename TemporalValue<kType>::type;
  const int lane = lane_id();
  const int my_word = lane >> 5;
  const int my_shift = (lane & 31) * 2;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + 2 * kTemporalSteps - 1) / (2 * kTemporalSteps);
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    uint64_t vw[kTemporalSteps][2];   // the step's two validity words (wave-uniform; a word past the last one reads as zero)
    T v[kTemporalSteps][2];
#pragma unroll
    for (int k = 0; k < kTemporalSteps; ++k) {
      const int64_t w0 = (s * kTemporalSteps + k) * 2;
      vw[k][0] = load_word(valid, w0);
      vw[k][1] = load_word(valid, w0 + 1);
      const int64_t row0 = (w0 << 6) + lane * 2;
      v[k][0] = v[k][1] = 0;
      if (row0 + 2 <= n) {
        __builtin_memcpy(&v[k][0], in + row0, 2 * sizeof(T));
      } else if (row0 < n) {
        v[k][0] = in[row0];
      }
    }
#pragma unroll
    for (int k = 0; k < kTemporalSteps; ++k) {
      const int64_t w0 = (s * kTemporalSteps + k) * 2;
      const int64_t row0 = (w0 << 6) + lane * 2;
      const uint64_t mine = (my_word ? vw[k][1] : vw[k][0]) >> my_shift;
      const bool ok0 = (mine & 1ull) != 0, ok1 = (mine & 2ull) != 0;
      I64x2 r;
      r.a = temporal_field<kType, kGroup>(ok0 ? v[k][0] : T{0}, component, week_start, count_from_one);
      r.b = temporal_field<kType, kGroup>(ok1 ? v[k][1] : T{0}, component, week_start, count_from_one);
      r.a = ok0 ? r.a : 0;   // (a null result slot: zero)
      r.b = ok1 ? r.b : 0;
      if (row0 + 2 <= n) {
        __builtin_memcpy(out + row0, &r, 16);
      } else if (row0 < n) {
        out[row0] = r.a;
      }
      if ((lane & 31) == 0 && out_valid != nullptr && w0 + my_word < nwords) out_valid[w0 + my_word] = my_word ? vw[k][1] : vw[k][0];
    }
  }
}

static int temporal_group(int component) {
  switch (component) {
    case ARX_TEMPORAL_YEAR: case ARX_TEMPORAL_QUARTER: case ARX_TEMPORAL_MONTH: case ARX_TEMPORAL_DAY: case ARX_TEMPORAL_DAY_OF_YEAR:
      return kGroupCivil;
    case ARX_TEMPORAL_ISO_YEAR: case ARX_TEMPORAL_ISO_WEEK: return kGroupIso;
    case ARX_TEMPORAL_DAY_OF_WEEK: return kGroupWeekday;
    case ARX_TEMPORAL_HOUR: case ARX_TEMPORAL_MINUTE: case ARX_TEMPORAL_SECOND: case ARX_TEMPORAL_MILLISECOND:
    case ARX_TEMPORAL_MICROSECOND: case ARX_TEMPORAL_NANOSECOND:
      return kGroupTime;
    default: return -1;
  }
}

// the reference's kernel lists: calendar fields of dates and timestamps, time-of-day fields of timestamps and times
static bool temporal_pair_ok(int group, int in_type) {
  if (group < 0 || in_type < ARX_TIME_DATE32 || in_type > ARX_TIME_TIME64_NS) return false;
  return group == kGroupTime ? in_type >= ARX_TIME_TIMESTAMP_S : in_type <= ARX_TIME_TIMESTAMP_NS;
}

template <int kType, int kGroup>
static void temporal_launch(unsigned grid, hipStream_t st, const ArxSpan* values, int64_t n, int component, int week_start,
                            int count_from_zero, void* out_data, void* out_validity) {
  using T = typename TemporalValue<kType>::type;
  hipLaunchKernelGGL((temporal_kernel<kType, kGroup>), dim3(grid), dim3(kBlock), 0, st, static_cast<const T*>(values->data) + values->offset,
                     make_bits(values->validity, values->offset, n), n, component, static_cast<uint32_t>(week_start),
                     count_from_zero ? 0u : 1u, static_cast<int64_t*>(out_data), static_cast<uint64_t*>(out_validity));
}

extern "C" {

int arx_temporal_component(int component, int in_type, const ArxSpan* values, int64_t length, int week_start, int count_from_zero,
                           void* out_data, void* out_validity, void* stream) {
  const int group = temporal_group(component);
  if (!temporal_pair_ok(group, in_type)) {
    set_error("arx_temporal_component: no kernel for component %d of input type %d (calendar fields: date32 .. timestamp[ns], "
              "time-of-day fields: timestamp[s] .. time64[ns])", component, in_type);
    return ARX_INVALID;
  }
  if (week_start < 1 || week_start > 7) {
    set_error("week_start must follow ISO convention (Monday=1, Sunday=7). Got week_start=%d", week_start);
    return ARX_INVALID;
  }
  if (length < 0) {
    set_error("arx_temporal_component: negative length %lld", static_cast<long long>(length));
    return ARX_INVALID;
  }
  if (values == nullptr) {
    set_error("arx_temporal_component: NULL values");
    return ARX_INVALID;
  }
  if (values->length != length) {
    set_error("arx_temporal_component: span length %lld is not length %lld", static_cast<long long>(values->length),
              static_cast<long long>(length));
    return ARX_INVALID;
  }
  if (length == 0) return ARX_OK;
  if (out_data == nullptr || values->data == nullptr) {
    set_error("arx_temporal_component: NULL %s", out_data == nullptr ? "out_data" : "data buffer of values");
    return ARX_INVALID;
  }
  if (out_validity == nullptr && values->validity != nullptr) {
    set_error("arx_temporal_component: NULL out_validity, but values has a validity bitmap");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  const int64_t nsteps = ceil_div(ceil_div(length, 64), 2 * kTemporalSteps);
  const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nsteps, kWavesPerBlock), kTemporalMaxBlocks)));
#define ARX_TEMPORAL_TYPE(TYPE, GROUP) \
  case TYPE: temporal_launch<TYPE, GROUP>(grid, st, values, length, component, week_start, count_from_zero, out_data, out_validity); break;
#define ARX_TEMPORAL_CALENDAR(GROUP)                                                                               \
  switch (in_type) {                                                                                               \
    ARX_TEMPORAL_TYPE(ARX_TIME_DATE32, GROUP) ARX_TEMPORAL_TYPE(ARX_TIME_DATE64, GROUP)                            \
    ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_S, GROUP) ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_MS, GROUP)                 \
    ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_US, GROUP) ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_NS, GROUP)                \
  }
  std::atomic<int64_t>* counter = nullptr;
  const char* kernel = "temporal_kernel";
  switch (group) {
    case kGroupCivil:
      ARX_TEMPORAL_CALENDAR(kGroupCivil)
      counter = &g_temporal_civil_launches;
      break;
    case kGroupIso:
      ARX_TEMPORAL_CALENDAR(kGroupIso)
      counter = &g_temporal_iso_launches;
      break;
    case kGroupWeekday:
      ARX_TEMPORAL_CALENDAR(kGroupWeekday)
      counter = &g_temporal_weekday_launches;
      break;
    default:
      switch (in_type) {
        ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_S, kGroupTime) ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_MS, kGroupTime)
        ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_US, kGroupTime) ARX_TEMPORAL_TYPE(ARX_TIME_TIMESTAMP_NS, kGroupTime)
        ARX_TEMPORAL_TYPE(ARX_TIME_TIME32_S, kGroupTime) ARX_TEMPORAL_TYPE(ARX_TIME_TIME32_MS, kGroupTime)
        ARX_TEMPORAL_TYPE(ARX_TIME_TIME64_US, kGroupTime) ARX_TEMPORAL_TYPE(ARX_TIME_TIME64_NS, kGroupTime)
      }
      counter = &g_temporal_time_launches;
      break;
  }
#undef ARX_TEMPORAL_CALENDAR
#undef ARX_TEMPORAL_TYPE
  ARX_CHECK_LAUNCH(kernel);
  counter->fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

}  // extern "C"

}  // namespace arx
