// The persistent token kernel's sticky error word and what the host does about it (DESIGN.md sections 3b, 3d, 3d2): the word's
// VOCABULARY, which token_kernel.h raises and llmk.hip reads, and the host's recovery POLICY as a state machine with no device code
// in it -- llmk.hip asks it what a completed launch's word means and carries that out (tk_perform); tests/test_tk_recover_cpu.py
// drives it from a stand-alone main with scripted events.  Plain C++, no HIP includes.
#ifndef LLMK_TK_RECOVER_H
#define LLMK_TK_RECOVER_H

namespace llmk {

// ---- the word.  The first cause is STORED, the marks are OR-ed in behind it; the low byte is detail (an exchange epoch or a layer)
constexpr unsigned TK_ERR_SPIN_GATHER = 0x100u;   // a bounded spin ran out: the service wave's gather (+ epoch & 0xff) ...
constexpr unsigned TK_ERR_SPIN_QKV = 0x200u;      // ... an attention CU's wait for q, k and v (+ layer) ...
constexpr unsigned TK_ERR_SPIN_PARTS = 0x300u;    // ... the head's CU waiting for the other attention parts (+ layer) ...
constexpr unsigned TK_ERR_SPIN_COOP = 0x400u;     // ... a q4_0 kernel's cooperative gather (+ epoch & 0xff)
constexpr unsigned TK_ERR_DRAINED = 0x1000u;      // mark: a workgroup saw the word raised and drained instead of spinning on
constexpr unsigned TK_ERR_NO_FINITE = 0x2000u;    // mark, added to a CLEAR word only: no finite logit among the candidates of a greedy fold
constexpr unsigned TK_ERR_RANGE = 0x4000u;        // a range event: an activation beyond the f16 image of a q4_0 kernel's x (+ epoch & 0xff)
constexpr unsigned TK_ERR_NOT_RANGE = 0x2f00u;    // no-finite-candidate and every spin class: a word with one of these is not a range event alone
// a range event and nothing else (drained or not): this position's activations did not fit, the kernel itself is sound
constexpr bool tk_range_only(unsigned code) { return (code & TK_ERR_RANGE) != 0 && (code & TK_ERR_NOT_RANGE) == 0; }
// what the kernel did, for the message of a retirement
constexpr const char* tk_err_words(unsigned code) {
    return (code & TK_ERR_NO_FINITE) ? "found no finite logit among its candidates"
         : (code & TK_ERR_RANGE)     ? "met an activation beyond the f16 range of its matrix-core operands"
                                     : "timed out waiting for its peer workgroups";
}

// ---- the q4_0 kernels' scale records (token_kernel.h tk_qsc) as the host filters them: {max|xb|, max|hb|, tag of x, tag of y}, the
// tags positions as int bits.  Every field whose tag is not `keep` and that is not already empty goes back to zero, value and tag
// (invariant R: a field tagged p holds position p's maximum of the sequence actually fed).  true: something changed
struct TkQscRecord { float x, y, z, w; };
inline bool tk_qsc_filter(TkQscRecord* rec, int n, int keep) {
    bool dropped = false;
    for (TkQscRecord* r = rec; r != rec + n; ++r) {
        int tz, tw;
        __builtin_memcpy(&tz, &r->z, sizeof(int));
        __builtin_memcpy(&tw, &r->w, sizeof(int));
        if (tz != keep && (tz != 0 || r->x != 0.f)) { r->x = r->z = 0.f; dropped = true; }
        if (tw != keep && (tw != 0 || r->y != 0.f)) { r->y = r->w = 0.f; dropped = true; }
    }
    return dropped;
}

// ---- the policy of one context
// Positions with a range event are redone ONE AT A TIME on the multi-kernel path and the kernel stays in use (one such position used
// to cost the context a third of its rate for good); TK_RANGE_LIMIT of them in a row retire it after all: a model it cannot hold
constexpr int TK_RANGE_LIMIT = 4;
constexpr int TK_KEEP_ALL = -1;      // no record tag to filter by: the records stay as they are

enum class TkVerdict {
    CLEAN,          // nothing to do
    NO_FINITE,      // clear the word: the logits in front of a greedy fold held no finite value, nothing of the kernel's is at fault
    REDO,           // clear the word, keep the kernel; the caller does this position on the multi-kernel path
    RETIRE          // clear the word and retire the kernel; the caller does this position on the multi-kernel path
};

struct TkRecovery {
    bool retired = false;       // set by whoever carries a RETIRE out: the context stays on the multi-kernel path (tk_setup_all)
    int range_events = 0;       // range events of single passes on this context, ever
    int range_run = 0;          // ... and IN A ROW: a clean position resets it wherever it ran
    int last_pos = 0;           // the position of the last launch that may have left records, 0: none since they were cleared

    // a position ran clean: a later range event is not "in a row" with an earlier one
    void clean() { range_run = 0; }
    // The records were zeroed -- llmk_reset, llmk_prefill and llmk_score (pf_run), tk_setup: no position before the next launch.
    // Neither count is touched: llmk_reset starts a new sequence on the same model, and it is the model the counts are about
    void cleared() { last_pos = 0; }

    // In front of a token-kernel launch at pos (q4: a q4_0 shape, the only ones with records).  A launch that continues the launch
    // before it finds its own buffer tagged pos - 2 or older, which nobody takes for history: TK_KEEP_ALL.  Any other launch -- the same
    // position again with another token, a rewind, a jump -- may find tags >= pos there that an earlier sequence left, and if it meets
    // an event the layers behind it keep them for position pos + 1 to read: keep only tag pos - 1, which its own sequence shares
    int before_launch(int pos, bool q4) {
        if (!q4) return TK_KEEP_ALL;
        const int keep = pos == last_pos + 1 ? TK_KEEP_ALL : pos - 1;
        last_pos = pos;
        return keep;
    }

    // the word one launch with one sync left (token_pass).  first_event: the context's first range event, worth a message
    struct Single { TkVerdict what; bool first_event; };
    Single single(unsigned err) {
        if (err == 0) { clean(); return {TkVerdict::CLEAN, false}; }
        if (!tk_range_only(err) || range_run + 1 >= TK_RANGE_LIMIT) return {TkVerdict::RETIRE, false};
        ++range_run;
        return {TkVerdict::REDO, range_events++ == 0};
    }

    // The word a drained speculative launch left on the device (spec_settle), or the host's copy of it (fa_deliver).  The launch BEHIND
    // a position raises NO_FINITE over that position's candidates; anything else is a launch's own trouble
    static TkVerdict settled(unsigned err) {
        return err == 0 ? TkVerdict::CLEAN : (err & TK_ERR_NO_FINITE) ? TkVerdict::NO_FINITE : TkVerdict::RETIRE;
    }

    // The end of n pipelined launches from pos0, `done` of whose ids arrived (decode_run).  Not clean: every launch behind the first
    // trouble drained on the sticky word, and the call resumes position by position at `resume`, where single() counts and redoes
    // what needs it -- the limit is not consulted here.  The launches queued behind a range event ran on its debris and may have left
    // records of it under their own positions: only the record of the last position whose id arrived is worth keeping (pos0 - 1
    // with done = 0: nothing of this call's).  Positions in front of the trouble ran clean
    struct Pipelined { TkVerdict what; int keep; int resume; };
    Pipelined pipelined_end(int pos0, int n, int done, unsigned err) {
        if (err == 0 && done == n) {
            clean();
            last_pos = pos0 + n - 1;
            return {TkVerdict::CLEAN, TK_KEEP_ALL, pos0 + n};
        }
        if (done > 0) clean();
        if (!tk_range_only(err)) return {TkVerdict::RETIRE, TK_KEEP_ALL, pos0 + done};
        last_pos = pos0 + done - 1;
        return {TkVerdict::REDO, pos0 + done - 1, pos0 + done};
    }
};

}  // namespace llmk

#endif  // LLMK_TK_RECOVER_H
