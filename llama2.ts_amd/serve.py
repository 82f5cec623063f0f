"""Continuous batching over the mixed step (runtime.Context.step_batch, include/llama2_hip.h: l2_step_batch).

Every request runs exactly the reference's loop (llama2.ts:462-500): BOS (1) fed at position 0, then the prompt forced, then one pick
per position (temperature 0: argmax; else one xorshift* draw from the request's own rng state), while pos < steps; a pick of BOS ends
the request and is not fed.  The fed stream is [1, prompt..., picks...] at positions 0, 1, ..., so the first pick comes from the logits
at position len(prompt).

Each request holds one slot (a reserved sequence: sequences 0 .. slots-1) from admission to its end.  Each step is one step_batch call:
one decode row per generating request, then prompt chunks of the oldest admitted requests that are still in their prompt, up to
max_rows rows in all.  A chunk's rows are known tokens; when the chunk ends at the prompt's last position its pick is the request's
first sampled token, otherwise it is fed with temperature 0 and its pick is thrown away (no draw).  Requests are admitted first come,
first served; a finished request's slot goes to the next waiting one, which restarts the slot at position 0.  The scheduler is plain
Python and deterministic for a given submission order; `ctx` is any object with step_batch (and get_option / cfg.seq_len, or pass
slots / seq_len).

A request submitted with logprobs=k (0 .. 20) gets, for each of its picks (the BOS pick included), the pick's log-probability under the
model's unscaled logits and the k most likely tokens with theirs, in Result.logprobs.  Only a step that holds such a request calls the
logprobs form of the step (l2_step_batch_logprobs), which leaves picks, rng states and caches exactly as the plain step does.

A request queued by submit_constrained or submit_n with allowed= and / or logit_bias= has every one of its picks constrained
(include/llama2_hip.h: l2_step_batch_constrained): `allowed` is an iterable of token ids (the same set for every pick) or a callable f(tokens_fed) -> iterable
of ids, or None for "anything" -- called once per real pick with every token of the request fed up to and including that step's, the
context the pick continues; `logit_bias` is a {id: value} dict added to the logits of every pick.  Picks, kept logits and logprobs are
those of the constrained rows.  A constrained pick of BOS still ends the request: allowing BOS is how a grammar says "may stop here".
A prompt chunk whose pick is thrown away is never constrained.  The keywords reach ctx.step_batch only in a step with such a pick.

A request queued by submit_sampling or submit_n with repetition_penalty / presence_penalty / frequency_penalty / top_k / min_p has
every one of its picks made under them (include/llama2_hip.h: l2_step_batch_sampling).  The history the penalties count is every token of
the request fed so far, this step's included, without the BOS at position 0: the prompt plus the picks.  The penalties change the row
everything reads (kept logits and logprobs are the penalised row's); top_k and min_p change only what a sampling pick is drawn from.
A thrown-away pick carries none of them, and the keywords reach ctx.step_batch only in a step that holds a real pick of such a request.

Scheduler(ctx, ..., prefix_cache=True) does not feed a prompt prefix whose cache rows the device already holds (a cache row of position
p depends on tokens 0 .. p only).  The scheduler remembers per slot the tokens whose rows it holds (`resident`: what was fed since the
slot's last restart; a finished request's rows stay until the slot is restarted).  A request with known tokens K = [BOS] + prompt may
reuse min(common prefix of K and a slot's resident tokens, min(len(K), steps) - 1) rows: at least one known token is always fed, so
its picks, logits and logprobs come from the same rows of the same step forms and tokens_fed is the same list.  On admission it takes
the free slot whose OWN rows give the longest reuse (ties: the lowest index) and restarts it in place at that position, no copy at
all; if an active slot offers at least min_fork_rows rows more, it takes the free slot released longest ago instead and the rows are
copied into it (ctx.seq_fork, include/llama2_hip.h: l2_seq_fork) before the step.  Consecutive admissions with the same source and row
count share one seq_fork call.  submit_n queues n samples of one prompt: the first feeds it, the others wait until its rows are there
and take them by one fork.  Without prefix_cache nothing of this runs: slots are taken lowest index first and restarted at position 0.
"""
import collections

from . import runtime

BOS = 1


class Result:
    """A finished request: tokens_fed (every token fed to the transformer, in order), finish ("bos" or "steps"), the rng state after its
    last draw, with keep_logits the logits each pick was made from (one row per pick, the BOS pick included), and with logprobs=k one
    (lp, [(id, lp), ... k]) per pick: the pick's log-probability and the k most likely tokens'."""

    __slots__ = ("tokens_fed", "finish", "rng_state", "logits", "logprobs")

    def __init__(self, tokens_fed, finish, rng_state, logits=None, logprobs=None):
        self.tokens_fed, self.finish, self.rng_state, self.logits = tokens_fed, finish, rng_state, logits
        self.logprobs = logprobs

    def __repr__(self):
        return "Result(tokens_fed=%d tokens, finish=%r, rng_state=%d)" % (len(self.tokens_fed), self.finish, self.rng_state)


class _Request:
    def __init__(self, rid, prompt, steps, temperature, topp, seed, logprobs=None, allowed=None, logit_bias=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, top_k=0, min_p=0.0):
        self.rid = rid
        stop = prompt.index(BOS) if BOS in prompt else -1      # a forced BOS ends the reference's loop there (llama2.ts:497)
        self.prompt = prompt if stop < 0 else prompt[:stop]
        self.forced_bos = stop >= 0
        self.known = [BOS] + self.prompt        # tokens of positions 0 .. len(prompt), known before any pick
        self.steps, self.temperature, self.topp, self.rng = steps, float(temperature), float(topp), int(seed)
        self.slot = None
        self.fed = []                           # tokens fed so far; the next one goes to position len(fed)
        self.next = None                        # the next token to feed once the prompt is done (a pick)
        self.logits = []
        self.top = None if logprobs is None else int(logprobs)
        self.logprobs = []
        self.allowed = allowed if allowed is None or callable(allowed) else [int(t) for t in allowed]
        self.logit_bias = dict(logit_bias) if logit_bias else None
        self.repetition, self.presence, self.frequency = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
        self.top_k, self.min_p = int(top_k), float(min_p)
        self.leader = None                      # submit_n with prefix_cache: the sample that feeds the prompt this one waits for
        self.done = False

    @property
    def reuse_limit(self):
        """Rows a request may take from a cache: every known token that will be fed, but the last."""
        return min(len(self.known), self.steps) - 1

    @property
    def penalised(self):
        return self.repetition != 1.0 or self.presence != 0.0 or self.frequency != 0.0

    @property
    def in_prompt(self):
        return len(self.fed) < len(self.known)


def _common(a, b, limit):
    """Length of the common prefix of a and b, at most limit."""
    n = min(len(a), len(b), limit)
    if a[:n] == b[:n]:
        return n
    i = 0
    while a[i] == b[i]:
        i += 1
    return i


class Scheduler:
    def __init__(self, ctx, max_rows=64, keep_logits=False, slots=None, seq_len=None, prefix_cache=False, min_fork_rows=16):
        self.ctx = ctx
        self.slots = int(slots) if slots is not None else int(ctx.get_option(runtime.OPT_SEQS))
        self.seq_len = int(seq_len) if seq_len is not None else int(ctx.cfg.seq_len)
        if self.slots < 1:
            raise ValueError("no sequences reserved: call seq_reserve first")
        if max_rows < self.slots:
            raise ValueError("max_rows %d < %d slots: every generating request needs its decode row" % (max_rows, self.slots))
        self.max_rows = int(max_rows)
        self.keep_logits = bool(keep_logits)
        self.waiting = collections.deque()
        self.active = []                        # in admission order
        self.free = list(range(self.slots))
        self.results = {}
        self._next_id = 0
        self.calls = 0
        # prefix reuse: min_fork_rows = 16 is one MFMA row tile -- fewer rows ride in a tile the step pays for anyway
        self.prefix_cache = bool(prefix_cache)
        self.min_fork_rows = int(min_fork_rows)
        if self.min_fork_rows < 1:
            raise ValueError("min_fork_rows %d < 1" % self.min_fork_rows)
        self.resident = [[] for _ in range(self.slots)]      # per slot: the tokens whose cache rows it holds
        self.released = list(range(self.slots))              # the free slots, the one released longest ago first
        self.rows_fed = self.rows_reused = self.forks = 0
        self.admit_log = None                   # set to a list to get (rid, slot, rows reused, source slot or None) per admission

    def submit(self, prompt_ids, steps, temperature=0.0, topp=1.0, seed=1, logprobs=None):
        """Queue one request; returns its id.  steps <= seq_len (the reference's clamp is the caller's).  logprobs: None, or k in
        0 .. 20 -- the log-probability of each pick and the k most likely tokens' (Result.logprobs)."""
        return self._submit(prompt_ids, steps, temperature, topp, seed, logprobs).rid

    def submit_constrained(self, prompt_ids, steps, temperature=0.0, topp=1.0, seed=1, logprobs=None, allowed=None, logit_bias=None):
        """submit() with constraints on every pick of the request (submit's own parameter list is pinned by tests/test_fork_cpu.py).
        allowed: None, an iterable of ids, or a callable f(tokens_fed) -> iterable of ids or None; logit_bias: None or {id: value}
        (see the module's text)."""
        return self._submit(prompt_ids, steps, temperature, topp, seed, logprobs, allowed, logit_bias).rid

    def submit_sampling(self, prompt_ids, steps, temperature=0.0, topp=1.0, seed=1, logprobs=None, allowed=None, logit_bias=None,
                        repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, top_k=0, min_p=0.0):
        """submit_constrained() with sampling controls on every pick of the request: penalties on the tokens fed so far (1 / 0 / 0:
        off), and for a sampling request top_k (0: off) and min_p (0: off); see the module's text."""
        return self._submit(prompt_ids, steps, temperature, topp, seed, logprobs, allowed, logit_bias,
                            (repetition_penalty, presence_penalty, frequency_penalty, top_k, min_p)).rid

    def submit_n(self, prompt_ids, steps, seeds, temperature=0.0, topp=1.0, logprobs=None, allowed=None, logit_bias=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, top_k=0, min_p=0.0):
        """Queue len(seeds) samples of one prompt, each a request of its own with its own rng state; returns their ids.  With
        prefix_cache the first is admitted as any request; the others become admissible once its prompt rows are resident (all of
        [BOS] + prompt but the last token) and take them by one fork.  Once the first has fed its prompt they are ordinary waiting
        requests: if its rows are gone when a slot comes free, they feed the prompt themselves."""
        reqs = []
        for seed in seeds:
            r = self._submit(prompt_ids, steps, temperature, topp, seed, logprobs, allowed, logit_bias,
                             (repetition_penalty, presence_penalty, frequency_penalty, top_k, min_p))
            if reqs and self.prefix_cache:
                r.leader = reqs[0]
            reqs.append(r)
        return [r.rid for r in reqs]

    def _submit(self, prompt_ids, steps, temperature, topp, seed, logprobs, allowed=None, logit_bias=None, controls=(1.0, 0.0, 0.0, 0, 0.0)):
        steps = int(steps)
        if steps < 0 or steps > self.seq_len:
            raise ValueError("steps %d outside [0, seq_len=%d]" % (steps, self.seq_len))
        if temperature != temperature or topp != topp:
            raise ValueError("temperature / topp is NaN")
        if logprobs is not None and not 0 <= int(logprobs) <= 20:
            raise ValueError("logprobs %d outside [0, 20]" % int(logprobs))
        rep, pres, freq, top_k, min_p = controls
        if not (0.0 < rep < float("inf")) or not all(abs(v) < float("inf") for v in (pres, freq)):
            raise ValueError("repetition_penalty must be positive and finite, presence_penalty / frequency_penalty finite")
        if int(top_k) < 0 or not 0.0 <= min_p <= 1.0:
            raise ValueError("top_k %r < 0 or min_p %r outside [0, 1]" % (top_k, min_p))
        if (int(top_k) > 0 or min_p > 0.0) and temperature < 0.0:
            raise ValueError("top_k / min_p with a negative temperature")
        r = _Request(self._next_id, [int(t) for t in prompt_ids], steps, temperature, topp, seed, logprobs, allowed, logit_bias, *controls)
        self._next_id += 1
        self.waiting.append(r)
        return r

    @property
    def idle(self):
        return not self.waiting and not self.active

    def _finish(self, r, how, done):
        res = Result(r.fed, how, r.rng, r.logits if self.keep_logits else None, None if r.top is None else r.logprobs)
        self.results[r.rid] = done[r.rid] = res
        r.done = True
        if r.slot is not None:
            self.active.remove(r)
            self.free.append(r.slot)
            self.free.sort()
            self.released.append(r.slot)
            if self.prefix_cache:
                self.resident[r.slot] = list(r.fed)      # (the caller owns the Result's list)

    def _admit(self, done):
        if not self.prefix_cache:
            while self.waiting and self.free:
                r = self.waiting.popleft()
                if r.steps == 0:                     # while (pos < steps) never runs
                    self._finish(r, "steps", done)
                    continue
                r.slot = self.free.pop(0)
                self.released.remove(r.slot)
                self.active.append(r)
                if self.admit_log is not None:
                    self.admit_log.append((r.rid, r.slot, 0, None))
            return
        forks = []                               # [source, rows, destinations], in admission order
        held = []                                # samples still waiting for their first one's prompt rows: they keep their place
        while self.waiting and self.free:
            r = self.waiting.popleft()
            if r.leader is not None and not r.leader.done and len(r.leader.fed) < r.reuse_limit:
                held.append(r)
                continue
            if r.steps == 0:
                self._finish(r, "steps", done)
                continue
            rows, src = self._place(r)
            r.fed = r.known[:rows]
            self.resident[r.slot] = r.fed
            self.rows_reused += rows
            self.active.append(r)
            if src is not None:
                if forks and forks[-1][0] == src and forks[-1][1] == rows:
                    forks[-1][2].append(r.slot)
                else:
                    forks.append([src, rows, [r.slot]])
            if self.admit_log is not None:
                self.admit_log.append((r.rid, r.slot, rows, src))
        self.waiting.extendleft(reversed(held))
        for src, rows, dsts in forks:
            self.ctx.seq_fork(src, dsts, rows)
            self.forks += 1

    def _place(self, r):
        """Give r its slot; returns (rows it reuses, the active slot they are to be copied from or None when they are its slot's own)."""
        lim = r.reuse_limit
        own, slot = -1, None
        for s in self.free:                      # ascending: ties go to the lowest index
            n = _common(r.known, self.resident[s], lim)
            if n > own:
                own, slot = n, s
        rows, src = own, None
        for a in self.active:
            n = _common(r.known, self.resident[a.slot], lim)
            if n >= own + self.min_fork_rows and (n > rows or (n == rows and a.slot < src)):
                rows, src = n, a.slot
        if src is not None:
            slot = self.released[0]
        self.free.remove(slot)
        self.released.remove(slot)
        r.slot = slot
        return rows, src

    def step(self):
        """One step_batch call over the admitted requests; returns {rid: Result} of those that finished in it."""
        done = {}
        self._admit(done)
        if not self.active:
            return done
        rows = []                                # (request, tokens, pos0, picks_count)
        for r in self.active:
            if not r.in_prompt:
                rows.append((r, [r.next], len(r.fed), True))
        budget = self.max_rows - len(rows)
        for r in self.active:
            if budget <= 0:
                break
            if r.in_prompt:
                p = len(r.fed)
                e = min(len(r.known), r.steps, p + budget)
                # the chunk's last row is the prompt's last position: its pick is the request's first real one
                rows.append((r, r.known[p:e], p, e == len(r.known) and not r.forced_bos))
                budget -= e - p
        seqs = [r.slot for r, _, _, _ in rows]
        temp = [r.temperature if real else 0.0 for r, _, _, real in rows]
        topp = [r.topp for r, _, _, _ in rows]
        rng = [r.rng for r, _, _, _ in rows]
        ks = [r.top for r, _, _, _ in rows if r.top is not None]
        extra = {"logprobs": max(ks)} if ks else {}
        # constraints of the real picks (a callable sees the tokens fed up to and including this step's); a thrown-away pick has none
        masks = [(r.allowed(r.fed + t) if callable(r.allowed) else r.allowed) if real else None for r, t, _, real in rows]
        bias = [r.logit_bias if real else None for r, _, _, real in rows]
        if any(m is not None for m in masks):
            extra["allowed"] = masks
        if any(b is not None for b in bias):
            extra["logit_bias"] = bias
        # sampling controls of the real picks: the history is what the request has fed after BOS, this step's tokens included
        pen = [real and r.penalised for r, _, _, real in rows]
        if any(pen):
            extra["history"] = [(r.fed + t)[1:] if on else None for (r, t, _, _), on in zip(rows, pen)]
            for key, attr, off in (("repetition_penalty", "repetition", 1.0), ("presence_penalty", "presence", 0.0), ("frequency_penalty", "frequency", 0.0)):
                col = [getattr(r, attr) if on and getattr(r, attr) != off else None for (r, _, _, _), on in zip(rows, pen)]
                if any(v is not None for v in col):
                    extra[key] = col
        for key, attr in (("top_k", "top_k"), ("min_p", "min_p")):
            col = [getattr(r, attr) if real and r.temperature != 0.0 and getattr(r, attr) > 0 else None for r, _, _, real in rows]
            if any(v is not None for v in col):
                extra[key] = col
        out = self.ctx.step_batch(seqs, [t for _, t, _, _ in rows], [p for _, _, p, _ in rows], temperature=temp, topp=topp, rng=rng,
                                  logits=self.keep_logits, **extra)
        self.calls += 1
        self.rows_fed += sum(len(t) for _, t, _, _ in rows)
        picks, rng_after = out[0], out[1]
        lps = out[-1] if ks else None
        for i, (r, toks, p, real) in enumerate(rows):
            r.fed.extend(toks)
            if real:
                if r.temperature != 0.0:
                    r.rng = int(rng_after[i])
                if self.keep_logits:
                    r.logits.append(out[2][i])
                if r.top is not None:
                    r.logprobs.append((float(lps[0][i]), [(int(lps[1][i][q]), float(lps[2][i][q])) for q in range(r.top)]))
                nxt = int(picks[i])
            elif r.in_prompt:
                nxt = r.known[len(r.fed)]
            elif r.forced_bos:
                nxt = BOS
            else:
                nxt = None                       # stopped by steps inside the prompt
            if nxt == BOS:
                self._finish(r, "bos", done)
            elif len(r.fed) >= r.steps:
                self._finish(r, "steps", done)
            else:
                r.next = nxt
        self._admit(done)
        return done

    def run(self):
        """Step until every submitted request has finished; returns {rid: Result} of every request finished so far."""
        while not self.idle:
            self.step()
        return dict(self.results)
