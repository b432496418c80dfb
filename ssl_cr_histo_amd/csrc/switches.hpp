// The SSLCR_* environment switches of the library: one table (switches.cpp), one reader, one listing (sslcr_switch_info).
// A site asks sw::on(sw::PP64) or sw::value(sw::WG_STAGGER) and keeps the comment that says why its switch exists; the name, the
// parse rule, the default, the moment of reading and the meaning are the row's.  No other file of csrc/ reads the environment.
#pragma once

namespace sslcr {
namespace sw {

// one per row of the table, in the table's order (switches.cpp holds the two together by a static_assert)
enum Id {
  PP64, H16_TW8, H16_RAW, S2, S2D, S2W, WG_DMA, WGRAD_WIDE,                                                  // routing
  GEMM_LDS, STEM_POOL_FORM, POOL_BANDS, WG_STAGGER,                                                          // form
  SEGMENTS, BN_PAIR, BN_PAIR_G, YBITS, UNFOLD_EVAL, STEM_POOL, BN_ONE_LAUNCH, FUSE_STEM_BWD, COMM_SELFTEST,  // engine
  BN_REPEAT, EW_CAP,                                                                                         // measurement
  COUNT
};

// How a row reads the string e that its variable holds.  Unset (e == NULL) is the row's default under every rule.
enum Rule {
  ATOI,     // on = atoi(e) != 0: "", "off" and " 0" turn a switch OFF, "01", "2" and "-1" leave it on
  LEAD0,    // off only when e[0] == '0': "", "off" and " 0" leave it ON, "01" and "00" turn it off
  INT,      // value = atoi(e) (EW_CAP: strtol), then held to the row's [lo, hi]
  PRESENT,  // on = set at all, the empty string included
};
// PROCESS: parsed once per process, thread-safely, at the first query of ANY switch -- after that a query is an array read, and a
// putenv is no longer seen.  CALL: parsed at every query (the entry point that asks is named in the row's meaning).
enum When { PROCESS, CALL };

struct Row {
  Id id;
  const char* name;      // with its prefix: "SSLCR_PP64"
  Rule rule;
  long dflt, lo, hi;     // lo, hi: INT rows, applied to a set value only
  When when;
  const char* group;     // "routing" | "form" | "engine" | "measurement"
  const char* meaning;
};
struct Value { bool set; long v; };   // v: 0 / 1 for the boolean rules

const Row& row(int i);               // 0 <= i < COUNT
Value get(Id id);
inline bool on(Id id) { return get(id).v != 0; }
inline long value(Id id) { return get(id).v; }
inline bool is_set(Id id) { return get(id).set; }

}  // namespace sw
}  // namespace sslcr
