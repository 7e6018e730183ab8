// kbin_words.h -- the counter words host and kernels share: the one definition
// of totals, gcount, misc, flat_n and pstat (kbin_internal.h includes it).
// Positions are fixed; a word that serves several phases has one name per
// meaning, with its lifetime.
#pragma once

namespace kb {

// ---- totals (u64, KB_TOTALS words; kb_ctx::totals, read back into h_totals)
constexpr int T_ENTRIES = 0;      // kept entries (bins_final / the table engine's runs pass, until kb_reset)
constexpr int T_IDS = 1;          // their ids
constexpr int T_BINS = 2;         // bins (the table engine: runs = distinct keys), until the next finalize
constexpr int T_BIN_OVER = 3;     // bins (runs) past the descriptors' capacity; 0 = none
constexpr int T_GCOUNT = 4;       // BinArgs::gcount = totals + T_GCOUNT: the G_* words below (bin kernels)
constexpr int T_WORK = 7;         // the bin kernel's work counter (device only)
constexpr int T_KMERS = 8;        // N: k-mer occurrences of the record pass
constexpr int T_RECORDS = 9;      // R: the one-pass record kernel's allocation counter
constexpr int T_STAGE = 10;       // stage allocation (bin plan, bin kernel)
constexpr int T_TAB_KEYS = 11;    // keys that entered a table (pre-filter learning)
// words 12..14, record pass until the bin plan (bucket_stats):
constexpr int T_REC_SUM = 12;     //   records summed over the buckets (R)
constexpr int T_REC_MAX = 13;     //   the largest bucket
constexpr int T_REC_STATUS = 14;  //   misc[M_REC_STATUS], so the pass reads back in one copy
// words 12..13, after bins_final until the finalize returns:
constexpr int T_HEAVY = 12;       //   heavy bins published (flat_n[FN_BINS])
constexpr int T_QUEUED = 13;      //   list items queued (*lq_n)
// words 12..13, after the finalize: kb_digest's two output words
constexpr int T_DIGEST = 12;
// the report block (bins_final with a deferred tail: the finalize's stats in one copy)
constexpr int T_REPORT = 16;                 // the low words are [0, T_REPORT)
constexpr int T_PSTAT = T_REPORT;            // pstat[0 .. KB_PSTAT)
constexpr int T_MISC_PAIRS = 28;             // misc[0 .. M_REPORTED) packed in pairs, low word first
constexpr int KB_TOTALS = 32;
// host only: binned_read_records' two-pass scan lands R here in h_totals
constexpr int HT_SCAN_R = 7;
// gcount (u64; totals + T_GCOUNT)
constexpr int G_PACKED = 0;    // entries << 32 | ids, allocated by the bins' prunes
constexpr int G_COUNTED = 1;   // sum of the counts before the prune (the invariant: == N)
constexpr int G_DISTINCT = 2;  // distinct keys before the prune

// ---- misc (u32, KB_MISC words; kb_ctx::misc, read back into h_misc)
constexpr int M_REC_STATUS = 0;  // status of the record pass and the bucket ordering; the table engine's status
constexpr int M_DISTINCT = 1;    // the table engine's distinct-key counter
constexpr int M_BIN_STATUS = 2;  // the bin kernels' status (BinArgs::status)
constexpr int M_LONG_N = 4;      // [2] the list kernels' long-list queue lengths (ListArgs::long_n)
constexpr int M_REPORTED = 6;    // words [0, M_REPORTED) are cleared, read back and reported by a finalize
constexpr int M_ALPHABET = 12;   // the pack kernel's sticky alphabet status (kb_submit until kb_reset)
constexpr int KB_MISC = 16;
constexpr int T_REPORT_END = T_MISC_PAIRS + M_REPORTED / 2;  // the report block is totals[T_REPORT, T_REPORT_END)
// host only: the radix sort's error word (os_aux[OS_AUX_ERR]) lands here in h_misc
constexpr int HM_RADIX_ERR = 8;
// os_aux (u32): [0, 4 * 256) digit histograms -> bases, [1024, 1028) tickets, then the error word
constexpr int OS_AUX_TICKETS = 4 * 256, OS_AUX_ERR = OS_AUX_TICKETS + 4, OS_AUX_WORDS = OS_AUX_TICKETS + 8;

// ---- flat_n (u64, KB_FLAT_N words, zeroed per attempt; BinArgs::flat_n)
constexpr int FN_BINS = 0;     // heavy / split bins published
constexpr int FN_POOL = 1;     // offset-pool allocation (BinArgs::flat_octr)
constexpr int FN_BUILD = 2;    // build items (record chunks)
constexpr int FN_COUNT = 3;    // (claim counters of the count and scatter passes: no longer used)
constexpr int FN_SCATTER = 4;
constexpr int FN_SWEEP = 5;    // phase 1's item claims
constexpr int FN_STAGED = 6;   // bins whose lists are written LDS-staged
constexpr int KB_FLAT_N = 8;

// ---- pstat (u64, KB_PSTAT words, zeroed per attempt; BinArgs::pstat -> kb_timing):
// path counters, one atomic per bin or partition
constexpr int PS_HEAVY = 0;       // heavy bins published as flat lists
constexpr int PS_SPLIT = 1;       // split bins published
constexpr int PS_PARTS = 2;       // partitions swept to their prune
constexpr int PS_REDO = 3;        // partitions redone split (overflow)
constexpr int PS_DEPTH = 4;       // deepest partition depth (max)
constexpr int PS_PREFILTERED = 5; // keys kept out by the pre-filter
constexpr int PS_OFFSET = 6;      // offset-range partitions
constexpr int PS_FLAT = 7;        // partitions swept from flat lists
constexpr int PS_PF_LIGHT = 8;    // light pre-filtered bins
constexpr int PS_RANKED = 9;      // ranked bins
constexpr int PS_BITMAP = 10;     // partitions emitted from rank bitmaps
constexpr int KB_PSTAT = 11;

static_assert(T_GCOUNT + G_DISTINCT < T_WORK, "gcount's words end below the work counter");
static_assert(T_REC_STATUS < T_REPORT && T_TAB_KEYS < T_REC_SUM, "the low words end below the report block");
static_assert(T_PSTAT + KB_PSTAT <= T_MISC_PAIRS, "pstat ends below the misc pairs");
static_assert(T_REPORT_END <= KB_TOTALS && M_REPORTED % 2 == 0, "the misc pairs fit");
static_assert(M_LONG_N + 2 <= M_REPORTED && M_REPORTED <= HM_RADIX_ERR && HM_RADIX_ERR < M_ALPHABET &&
                  M_ALPHABET < KB_MISC,
              "misc: reported words, the host's radix word, the alphabet word");
static_assert(FN_STAGED < KB_FLAT_N && PS_BITMAP < KB_PSTAT, "flat_n and pstat hold their words");

}  // namespace kb
