// llmk_forward keeps the next greedy position in flight: the POLICY, as a state machine with no device
// code in it -- llmk.hip asks it what a call should do and carries that out; tests/test_forward_ahead_cpu.py drives it from a
// stand-alone main with scripted call sequences.  Plain C++, no HIP includes.
//
// A caller that feeds back the first maximum of the logits it just received (llama2.f90:376-402 at -t 0) is recognised from the
// host's side first -- two calls in a row whose token is that maximum ARM the machine -- and from then on the device's own greedy
// token decides: the launch for position q takes its token from position q - 1's classifier candidates and publishes the id it
// took; a call forward(tok, q) whose tok is that id is a HIT and finds its result under way, anything else is a MISS, which drains
// the stream, runs the call as if nothing had been launched, and backs off.  Whether a speculative result is used is decided by the
// published id alone; the host's scan of the logits only decides whether to try.
#ifndef LLMK_FORWARD_AHEAD_H
#define LLMK_FORWARD_AHEAD_H

namespace llmk {

// the device's rule (token_kernel.h tk_token, cand_resolve_kernel): the first maximum, and a NaN never wins; -1: no logit is
// greater than -inf
inline int fa_first_max(const float* v, int n) {
    float bv = -__builtin_inff();
    int bi = -1;
    for (int i = 0; i < n; ++i)
        if (v[i] > bv) { bv = v[i]; bi = i; }
    return bi;
}

struct ForwardAhead {
    static constexpr int ARM_STREAK = 2;            // agreements in a row that arm the machine
    static constexpr int BACKOFF_FIRST = 16;        // sequential calls that skip the comparison after a disagreement ...
    static constexpr int BACKOFF_MAX = 1024;        // ... doubling up to this: a caller that samples on the host scans a handful of times

    bool armed = false;         // ARMED: the launch for position `next` is in flight on the device's own token; else IDLE
    int next = 0;
    int last = 0;               // IDLE: the position whose logits the last call left in pinned memory (0: none)
    int streak = 0;
    int skip = 0;               // comparisons still to skip
    int backoff = 0;            // length of the running backoff (0: none yet)
    // {speculative launches, hits, misses} as llmk_forward_ahead_stats reports them, and the host scans
    int launches = 0, hits = 0, misses = 0, scans = 0;

    // IDLE: does forward(tok, pos) compare tok with the previous position's logits?  Only a call that continues the sequence
    // can; inside a backoff it counts down instead.
    bool scan_due(int pos) {
        if (armed || last == 0 || pos != last + 1) { streak = 0; return false; }
        if (skip > 0) { --skip; return false; }
        ++scans;
        return true;
    }
    // IDLE: what the comparison said.  true: this call arms -- it launches position pos itself in the greedy instantiation and
    // position pos + 1 behind it (never a position beyond S: the call at S has nothing to speculate on)
    bool scanned(bool agree, int pos, int S) {
        if (!agree) { disagree(); return false; }
        if (++streak < ARM_STREAK || pos >= S) return false;
        armed = true;
        next = pos + 1;
        ++launches;
        return true;
    }
    // ARMED: is this the call the launch in flight was made for?  (its token is then compared with the device's id)
    bool expects(int pos) const { return armed && pos == next; }
    // ARMED: the device's id was the caller's token.  true: launch position pos + 1 BEFORE waiting for pos; false: pos is S, the
    // machine goes IDLE with nothing in flight
    bool hit(int S) {
        ++hits;
        if (next + 1 <= S) { ++next; ++launches; return true; }
        armed = false;
        streak = 0;
        return false;
    }
    // ARMED: any other call -- another token, another position.  The caller drains the stream and runs the call as an IDLE one
    void miss() {
        ++misses;
        armed = false;
        last = 0;
        disagree();
    }
    // a call delivered position pos's logits (by whichever path): the next sequential call may be compared with them
    void ran(int pos) { last = pos; }
    // another entry point used the context, or a call failed: IDLE, and nothing to compare the next call with
    void interrupt() {
        armed = false;
        last = 0;
        streak = 0;
    }

private:
    void disagree() {
        streak = 0;
        backoff = backoff == 0 ? BACKOFF_FIRST : backoff >= BACKOFF_MAX / 2 ? BACKOFF_MAX : 2 * backoff;
        skip = backoff;
    }
};

}  // namespace llmk

#endif  // LLMK_FORWARD_AHEAD_H
