"""What the device sampler draws from, compiled once: the host side of generation's sampling options.
`Constraint`, `Grammar`, `Preference` and the compilers turn the options into host tables; `DrawPlan` is the one place
that calls them and makes every refusal for them, before any device work.  Each entry of generation.py builds one plan,
`DeviceDraw(plan, dev)` puts it on the session's device once, and the token loops, `_draw_token` and the scorers read
that object.  Nothing here needs a GPU, a DecodeSession or ops; only `DeviceDraw` creates device tensors."""
import copy

import numpy as np
import torch

# per-attribute sampler settings of forward_output_sampling (dqn_policy/model.py:281-286), attribute order
DQN_TEMPERATURE = (1.2, 1.0, 1.2, 1.0, 2.0, 5.0)
DQN_TOP_P = (0.9, 0.99, None, 0.9, 0.9, None)


class Constraint:
    """What a song may contain, attribute by attribute, enforced inside the device sampler
    (cwlt_sample_categorical_masked).  generate_batch / generate_stream / generate(batch_size=... | slots=...) take it
    as `constraints=`.

    allow: {attribute name (a key of word2event, e.g. "pitch"): events}, a static allowed set for every bar.
    per_bar: {attribute name: [events, events, ...]}, a schedule whose entry i applies to bar i + 1.
    Events are event names (values of word2event[attribute]) or class ids; a single name or id is one event.
    Bars follow the generation bar rule: the count starts at 1 and counts the Bar tokens of the prompt's rows after the
    first; a drawn row is constrained by the entry for the count BEFORE that row, and the count goes up after a row
    whose bar-beat class is a Bar class -- so the Bar token that opens bar c + 1 is still drawn under bar c's entry.
    Past the end of a schedule its last entry holds; cycle=True repeats the schedule instead.
    keep_neutral=True: in every attribute the constraint restricts, class 0 and every class named "CONTI" stay allowed
    (note rows carry 0 in tempo / chord / bar-beat, metrical rows 0 in pitch / duration / velocity and often CONTI in
    tempo / chord), so a pitch range or a chord set does not force every row to be a note or a beat.
    The draw: disallowed classes are -inf logits before the temperature, the max, the softmax and the nucleus (top_p is
    taken over the renormalised allowed distribution).  Draw keys are unchanged, so a constraint that allows every
    class gives bitwise the unconstrained songs.  Prompt rows are never constrained.
    Refused (ValueError): unknown attribute or event names, ids out of range, an empty allowed set, an attribute in both
    allow and per_bar."""

    def __init__(self, word2event, allow=None, per_bar=None, cycle=False, keep_neutral=True):
        self.keys = list(word2event.keys())
        self.n_class = [len(word2event[k]) for k in self.keys]
        self.cycle, self.keep_neutral = bool(cycle), bool(keep_neutral)
        allow = {} if allow is None else dict(allow)
        per_bar = {} if per_bar is None else dict(per_bar)
        both = sorted(set(allow) & set(per_bar))
        if both:
            raise ValueError("attribute %r is in both allow and per_bar" % both[0])
        self.static = {self._attr(name): self._allowed(word2event, name, ev) for name, ev in allow.items()}
        self.schedule = {}
        for name, entries in per_bar.items():
            a = self._attr(name)
            if isinstance(entries, (str, bytes)) or not hasattr(entries, "__len__") or len(entries) == 0:
                raise ValueError("per_bar[%r] must be a non-empty list with one collection of events per bar" % (name,))
            self.schedule[a] = [self._allowed(word2event, name, ev, i) for i, ev in enumerate(entries)]
        self.bar_attr = self.keys.index("bar-beat") if "bar-beat" in self.keys else None
        self.bar_ids = [] if self.bar_attr is None else \
            [i for i, e in word2event["bar-beat"].items() if e == "Bar"]

    def _attr(self, name):
        if name not in self.keys:
            raise ValueError("unknown attribute %r (attributes: %s)" % (name, ", ".join(map(str, self.keys))))
        return self.keys.index(name)

    def _allowed(self, word2event, name, events, bar=None):
        where = "%r" % (name,) if bar is None else "%r, bar %d" % (name, bar + 1)
        names = word2event[name]
        n = len(names)
        if isinstance(events, (str, bytes, int, np.integer)):
            events = [events]
        keep = np.zeros(n, dtype=bool)
        count = 0
        for ev in events:
            count += 1
            if isinstance(ev, (int, np.integer)) and not isinstance(ev, bool):
                if not 0 <= int(ev) < n:
                    raise ValueError("%s: class id %d out of range (%d classes)" % (where, int(ev), n))
                keep[int(ev)] = True
                continue
            ids = [i for i, e in names.items() if e == ev]
            if not ids:
                raise ValueError("%s: unknown event %r" % (where, ev))
            keep[ids] = True
        if count == 0:
            raise ValueError("%s: the allowed set is empty" % where)
        if self.keep_neutral:
            keep[0] = True
            keep[[i for i, e in names.items() if e == "CONTI"]] = True
        return keep

    def allowed(self, bar):
        """Per attribute, the (n_class,) bool array of classes allowed in bar `bar` (the count before the row)."""
        out = []
        i = max(int(bar) - 1, 0)
        for a, n in enumerate(self.n_class):
            if a in self.static:
                out.append(self.static[a])
            elif a in self.schedule:
                sch = self.schedule[a]
                out.append(sch[i % len(sch)] if self.cycle else sch[min(i, len(sch) - 1)])
            else:
                out.append(np.ones(n, dtype=bool))
        return out

    def mask_rows(self, bar_cond):
        """The device table of this constraint for songs that end at bar `bar_cond` -> (R, ceil(sum n_class / 32))
        uint32: row i is bar i + 1, class c of attribute a is bit sum(n_class[:a]) + c.  Without a schedule R = 1;
        cycle=True expands the schedule to bar_cond - 1 rows (no kept row is drawn at a count >= bar_cond); otherwise R
        is the longest schedule, cut at bar_cond - 1.  The device clamps to the last row."""
        last = max(1, int(bar_cond) - 1)
        if not self.schedule:
            R = 1
        elif self.cycle:
            R = last
        else:
            R = min(max(len(v) for v in self.schedule.values()), last)
        W = -(-sum(self.n_class) // 32)
        bits = np.zeros((R, W * 32), dtype=bool)
        for i in range(R):
            row = np.concatenate(self.allowed(i + 1))
            bits[i, :len(row)] = row
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(R, W)

    def can_end(self, bar0, bar_cond):
        """False when some bar in [bar0, bar_cond) allows no Bar class: a song there could never reach bar_cond."""
        if self.bar_attr is None or (self.bar_attr not in self.static and self.bar_attr not in self.schedule):
            return True
        for b in range(int(bar0), int(bar_cond)):
            if not self.allowed(b)[self.bar_attr][self.bar_ids].any():
                return False
        return True

    def violations(self, song, bar0=1):
        """Indices of the rows of `song` ((L, 6) drawn rows, e.g. generated[len(prompt):]) that break the constraint,
        the first row drawn at bar count bar0 (1 from scratch; a prompt's own count after a prompt)."""
        song = np.asarray(song, dtype=np.int64).reshape(-1, len(self.n_class))
        bad, b = [], int(bar0)
        bar_ids = set(self.bar_ids)
        for t, row in enumerate(song):
            ok = self.allowed(b)
            if any(not (0 <= int(c) < n and ok[a][int(c)]) for a, (c, n) in enumerate(zip(row, self.n_class))):
                bad.append(t)
            if self.bar_attr is not None and int(row[self.bar_attr]) in bar_ids:
                b += 1
        return bad


def compile_constraints(constraints, n_songs, n_token, bar_cond, bar0s, max_tokens):
    """The device table of `constraints` (one Constraint for every song, or a list of n_songs entries, None =
    unconstrained) -> None when no song is constrained, else (sched (n_songs, 2) int64 {first row, rows}, masks (R, W)
    uint32).  One Constraint object's rows are shared by all songs that use it; an unconstrained song has 0 rows.
    bar0s: each song's bar count before its first drawn row.  Without max_tokens a song whose bar-beat restriction
    allows no Bar class in some bar it can reach would never end: refused."""
    if isinstance(constraints, Constraint):
        constraints = [constraints] * n_songs
    elif isinstance(constraints, (list, tuple)):
        if len(constraints) != n_songs:
            raise ValueError("constraints: %d entries for %d songs" % (len(constraints), n_songs))
    else:
        raise ValueError("constraints must be a Constraint or a list of n_songs Constraint / None entries, got %s"
                         % type(constraints).__name__)
    if all(c is None for c in constraints):
        return None
    sched = np.zeros((n_songs, 2), dtype=np.int64)
    parts, rows, ends, total = [], {}, {}, 0
    for k, c in enumerate(constraints):
        if c is None:
            continue
        if not isinstance(c, Constraint):
            raise ValueError("constraints[%d] is a %s, not a Constraint or None" % (k, type(c).__name__))
        if list(c.n_class) != list(n_token):
            raise ValueError("constraints[%d] was built for classes %s, the model draws %s" % (k, c.n_class,
                                                                                            list(n_token)))
        if id(c) not in rows:
            parts.append(c.mask_rows(bar_cond))
            rows[id(c)] = (total, len(parts[-1]))
            total += len(parts[-1])
        sched[k] = rows[id(c)]
        if max_tokens is None:
            key = (id(c), int(bar0s[k]))
            if key not in ends:
                ends[key] = c.can_end(bar0s[k], bar_cond)
            if not ends[key]:
                raise ValueError("constraints[%d] allows no Bar in some bar before bar_cond=%d: the song could never "
                                 "end (pass max_tokens, or allow a Bar class in every bar)" % (k, bar_cond))
    return sched, np.concatenate(parts)


class Grammar:
    """The row grammar of CW songs, enforced inside the device sampler (cwlt_sample_categorical_grammar).
    generate_batch / generate_stream / generate(batch_size=... | slots=...) / score_songs take it as `grammar=`.

    A row is exactly one of three kinds, decided by its class in attribute `bar_attr`:
      NOTE: bar_attr class 0; class 0 in every `metrical` attribute; any class but 0 in every `note` attribute;
      BAR:  a bar_attr class named "Bar"; class 0 everywhere else;
      BEAT: a bar_attr class Beat_<k>; any class but 0 (CONTI or a value) in every `metrical` attribute, class 0 in
            every `note` attribute.
    Position rule: each song carries `beat`: -1 after a Bar row, k after Beat_k, unchanged by note rows.  A Bar class
    is always allowed, Beat_k when k > beat, class 0 (a note) when beat >= 0: beats ascend within a bar and no note
    comes before a bar's first beat.  A prompt's rows are not constrained; they only move `beat`, from -1.
    The bar-beat class is drawn first, under (the song's Constraint row, if any) AND (the position rule); every other
    attribute under (constraint row) AND (the kind's row).  Masking, temperature, nucleus and keys are Constraint's.

    The neutral class is class id 0 (as in Constraint); beat indices are parsed from the names Beat_<k>, or given as
    beats={class id: index}.  Refused (ValueError): unknown attributes, an attribute in two roles, a bar_attr class that
    is neither class 0, "Bar" nor a beat, no Bar class at all."""

    NOTE, BAR, BEAT = 0, 1, 2

    def __init__(self, word2event, bar_attr="bar-beat", metrical=("tempo", "chord"),
                 note=("pitch", "duration", "velocity"), beats=None):
        self.keys = list(word2event.keys())
        self.n_class = [len(word2event[k]) for k in self.keys]
        roles = [bar_attr] + list(metrical) + list(note)
        for name in roles:
            if name not in self.keys:
                raise ValueError("unknown attribute %r (attributes: %s)" % (name, ", ".join(map(str, self.keys))))
        if len(set(roles)) != len(roles):
            raise ValueError("an attribute has two roles among bar_attr, metrical and note: %s" % (roles,))
        self.bar_attr = self.keys.index(bar_attr)
        self.metrical = [self.keys.index(k) for k in metrical]
        self.note = [self.keys.index(k) for k in note]
        beats = {} if beats is None else {int(c): int(k) for c, k in dict(beats).items()}
        names = word2event[bar_attr]
        n = self.n_class[self.bar_attr]
        order = np.full(n, -3, dtype=np.int32)
        order[0] = -2
        for c in range(1, n):
            name = names[c]
            if c in beats:
                if beats[c] < 0:
                    raise ValueError("beats[%d] = %d: a beat index is >= 0" % (c, beats[c]))
                order[c] = beats[c]
            elif name == "Bar":
                order[c] = -1
            elif isinstance(name, str) and name.startswith("Beat_") and name[5:].isdigit():
                order[c] = int(name[5:])
            else:
                raise ValueError("%s class %d (%r) is neither class 0, \"Bar\" nor Beat_<k>: pass beats={class id: "
                                 "index}" % (bar_attr, c, name))
        for c in beats:
            if not 1 <= c < n:
                raise ValueError("beats: class id %d outside 1..%d" % (c, n - 1))
        if not (order == -1).any():
            raise ValueError("%s has no class named \"Bar\"" % (bar_attr,))
        self.order = order
        self.bar_ids = [int(c) for c in np.nonzero(order == -1)[0]]

    def kind(self, c):
        """The kind of a row whose bar_attr class is c (NOTE / BAR / BEAT), None for a class outside the attribute."""
        if not 0 <= int(c) < len(self.order):
            return None
        o = int(self.order[int(c)])
        return self.NOTE if o == -2 else self.BAR if o == -1 else self.BEAT

    def allowed(self, kind):
        """Per attribute, the (n_class,) bool array of classes a row of `kind` may carry (bar_attr: the kind's own
        classes; an attribute with no role: every class)."""
        out = []
        for a, n in enumerate(self.n_class):
            ok = np.ones(n, dtype=bool)
            if a == self.bar_attr:
                ok = np.array([self.kind(c) == kind for c in range(n)])
            elif (a in self.note and kind == self.NOTE) or (a in self.metrical and kind == self.BEAT):
                ok[0] = False
            elif a in self.note or a in self.metrical:
                ok[1:] = False
            out.append(ok)
        return out

    def position_allowed(self, beat):
        """The (n_class[bar_attr],) bool array of bar_attr classes the position rule allows at `beat`."""
        o, b = self.order.astype(np.int64), int(beat)
        return (o == -1) | ((o >= 0) & (o > b)) | ((o == -2) & (b >= 0))

    def tables(self):
        """The device tables -> (order (n_class[bar_attr],) int32: -2 class 0, -1 Bar, k >= 0 Beat_k;
        gram (3, ceil(sum n_class / 32)) uint32: rows NOTE, BAR, BEAT in the bit layout of Constraint.mask_rows)."""
        W = -(-sum(self.n_class) // 32)
        bits = np.zeros((3, W * 32), dtype=bool)
        for kind in (self.NOTE, self.BAR, self.BEAT):
            row = np.concatenate(self.allowed(kind))
            bits[kind, :len(row)] = row
        return self.order.copy(), np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(3, W)

    def beat_states(self, song, beat=-1):
        """The position before each row of `song` ((L, 6) rows) and after the last -> ((L,) int64, final), the first
        row met at `beat` (-1: the start of a bar, what a song starts from)."""
        song = np.asarray(song, dtype=np.int64).reshape(-1, len(self.n_class))
        c = song[:, self.bar_attr]
        inside = (c >= 0) & (c < len(self.order))
        o = np.where(inside, self.order.astype(np.int64)[np.where(inside, c, 0)], -3)
        # after row t: the order of the last Bar / Beat row up to t, `beat` when there is none
        last = np.maximum.accumulate(np.where(o >= -1, np.arange(len(song)), -1))
        after = np.where(last >= 0, o[np.maximum(last, 0)], int(beat))
        before = np.concatenate([[int(beat)], after[:-1]]).astype(np.int64)[:len(song)]
        return before, int(after[-1]) if len(song) else int(beat)

    def violations(self, song, n_prompt=0):
        """Indices of the rows of `song` ((L, 6), its first n_prompt rows a prompt: tracked, not checked) that break
        the kind table or the position rule."""
        song = np.asarray(song, dtype=np.int64).reshape(-1, len(self.n_class))
        before, _ = self.beat_states(song)
        c = song[:, self.bar_attr]
        inside = (c >= 0) & (c < len(self.order))
        o = np.where(inside, self.order.astype(np.int64)[np.where(inside, c, 0)], -3)
        ok = (o == -1) | ((o >= 0) & (o > before)) | ((o == -2) & (before >= 0))
        kind = np.where(o == -2, self.NOTE, np.where(o == -1, self.BAR, self.BEAT))
        sets = [self.allowed(k) for k in (self.NOTE, self.BAR, self.BEAT)]
        for a, n in enumerate(self.n_class):
            if a == self.bar_attr:
                continue
            x = song[:, a]
            table = np.stack([s[a] for s in sets])                     # (3, n_class[a])
            ok &= (x >= 0) & (x < n) & table[kind, np.clip(x, 0, n - 1)]
        return [int(t) for t in np.nonzero(~ok)[0] if t >= int(n_prompt)]


def compile_grammar(grammar, constraints, n_songs, n_token, bar_cond):
    """Grammar.tables() checked against the model's classes and the songs' constraints -> (order, gram).  Refused, so
    that no reachable draw has an empty allowed set: a constraint row (any bar the device table holds) that leaves some
    kind no class in some attribute, or allows no Bar class -- what the position rule always allows."""
    if not isinstance(grammar, Grammar):
        raise ValueError("grammar must be a Grammar, got %s" % type(grammar).__name__)
    if list(grammar.n_class) != list(n_token):
        raise ValueError("the grammar was built for classes %s, the model draws %s" % (grammar.n_class, list(n_token)))
    if isinstance(constraints, Constraint):
        constraints = [constraints]
    seen = set()
    kinds = [("note", grammar.allowed(Grammar.NOTE)), ("Bar", grammar.allowed(Grammar.BAR)),
             ("beat", grammar.allowed(Grammar.BEAT))]
    for c in constraints or []:
        if not isinstance(c, Constraint) or id(c) in seen:
            continue
        seen.add(id(c))
        if list(c.n_class) != list(n_token):
            continue                                                   # compile_constraints refuses it
        for i in range(len(c.mask_rows(bar_cond))):
            ok = c.allowed(i + 1)
            if not ok[grammar.bar_attr][grammar.bar_ids].any():
                raise ValueError("grammar: the constraint allows no Bar class in bar %d, the one class the position "
                                 "rule always allows" % (i + 1))
            for name, sets in kinds:
                for a, (x, y) in enumerate(zip(ok, sets)):
                    if a != grammar.bar_attr and not (x & y).any():
                        raise ValueError("grammar: in bar %d the constraint leaves a %s row no class of %r (class 0 "
                                         "must stay allowed where the kind carries it: keep_neutral=True)"
                                         % (i + 1, name, grammar.keys[a]))
    return grammar.tables()


def compile_alpha(alpha, n_songs, n_attr):
    """The blend weights of generation with a reference model -> the device table's host form, float32
    (1, n_attr) (every song) or (n_songs, n_attr).  alpha: a scalar; (n_songs,) one value per song; (1, n_attr) one per
    attribute; (n_songs, n_attr).  A one-dimensional alpha is always per song.  Entries are finite floats of any sign
    or size: 1 is the model, 0 the reference, above 1 extrapolates.  Refused (ValueError): any other shape, a
    non-finite or non-numeric entry."""
    n_songs, A = int(n_songs), int(n_attr)
    try:
        a = None if alpha is None else np.asarray(alpha, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None:
        raise ValueError("alpha must be a number or an array of numbers, got %s" % type(alpha).__name__)
    if a.ndim == 0:
        a = np.full((1, A), float(a))
    elif a.ndim == 1 and a.shape[0] == n_songs:
        a = np.repeat(a[:, None], A, axis=1)
    elif a.ndim != 2 or a.shape[1] != A or a.shape[0] not in (1, n_songs):
        raise ValueError("alpha must be a scalar, (n_songs,) = (%d,), (1, %d) or (%d, %d), got shape %s"
                         % (n_songs, A, n_songs, A, a.shape))
    with np.errstate(over="ignore"):
        out = a.astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError("alpha entries must be finite (in float32)")
    return np.ascontiguousarray(out)


class Preference:
    """What a song should rather contain: soft terms on the logits, added by cwlt_prefer_logits in front of the
    unchanged device samplers.  generate_batch / generate_stream / generate(batch_size=... | slots=...) /
    score_songs / policy_stats take it as `preferences=`.  A Constraint forbids; a Preference only moves mass.

    bias: {attribute name: {event name or class id: float}}, a static additive logit bias for every bar.
    per_bar: {attribute name: [{event: float}, ...]}, a schedule whose entry i applies to bar i + 1, under the generation
    bar rule exactly as Constraint states it: the count used is the one before the row, a Bar token is drawn under the
    bar it closes, past the end of a schedule its last entry holds, cycle=True repeats the schedule.  Classes not named
    get 0.  Event names and ids resolve as in Constraint.
    repeat: {attribute name: frequency} or {attribute name: (frequency, presence)}, the repetition penalty.  Each song
    carries `seen`, one f32 per class of every attribute (sum n_class wide, the sampler's column layout): after every
    row of the song, prompt rows included, seen = seen * decay + hit, hit 1 at the class the row carries in each
    attribute -- as a prompt's rows move the grammar's `beat` without being constrained.  The logit of class c != 0 of
    attribute a is lowered by frequency[a] * seen[c] + (presence[a] if seen[c] > 0 else 0).  Class 0 of every attribute,
    the neutral class every note row carries in tempo / chord / bar-beat and every metrical row in pitch / duration /
    velocity, is never penalised (its `seen` is still tracked).  decay in (0, 1]: 1 counts, below 1 forgets.
    Refused (ValueError): unknown attribute or event names, ids out of range, an attribute in both bias and per_bar, an
    empty per_bar list, any value not finite in float32 (a hard ban is a Constraint's job), decay outside (0, 1]."""

    def __init__(self, word2event, bias=None, per_bar=None, cycle=False, repeat=None, decay=1.0):
        self.keys = list(word2event.keys())
        self.n_class = [len(word2event[k]) for k in self.keys]
        self.cycle = bool(cycle)
        bias = {} if bias is None else dict(bias)
        per_bar = {} if per_bar is None else dict(per_bar)
        both = sorted(set(bias) & set(per_bar))
        if both:
            raise ValueError("attribute %r is in both bias and per_bar" % both[0])
        self.static = {self._attr(name): self._values(word2event, name, ev) for name, ev in bias.items()}
        self.schedule = {}
        for name, entries in per_bar.items():
            a = self._attr(name)
            if isinstance(entries, (str, bytes, dict)) or not hasattr(entries, "__len__") or len(entries) == 0:
                raise ValueError("per_bar[%r] must be a non-empty list with one {event: bias} mapping per bar" % (name,))
            self.schedule[a] = [self._values(word2event, name, ev, i) for i, ev in enumerate(entries)]
        A = len(self.keys)
        self.frequency, self.presence = np.zeros(A, dtype=np.float32), np.zeros(A, dtype=np.float32)
        for name, value in ({} if repeat is None else dict(repeat)).items():
            a = self._attr(name)
            pair = tuple(value) if isinstance(value, (tuple, list)) else (value, 0.0)
            if len(pair) != 2:
                raise ValueError("repeat[%r] must be a frequency or a (frequency, presence) pair" % (name,))
            self.frequency[a] = self._finite(pair[0], "repeat[%r]: the frequency penalty" % (name,))
            self.presence[a] = self._finite(pair[1], "repeat[%r]: the presence penalty" % (name,))
        self.decay = self._finite(decay, "decay")
        if not 0.0 < float(self.decay) <= 1.0:
            raise ValueError("decay must lie in (0, 1] (in float32), got %r" % (decay,))

    def _attr(self, name):
        if name not in self.keys:
            raise ValueError("unknown attribute %r (attributes: %s)" % (name, ", ".join(map(str, self.keys))))
        return self.keys.index(name)

    @staticmethod
    def _finite(value, what):
        try:
            with np.errstate(over="ignore"):
                v = np.float32(value)
        except (TypeError, ValueError):
            v = np.float32(np.nan)
        if isinstance(value, (bool, str, bytes)) or not np.isfinite(v):
            raise ValueError("%s must be a number finite in float32, got %r (a hard ban is a Constraint's job)"
                             % (what, value))
        return v

    def _values(self, word2event, name, events, bar=None):
        where = "%r" % (name,) if bar is None else "%r, bar %d" % (name, bar + 1)
        names = word2event[name]
        n = len(names)
        if not hasattr(events, "items"):
            raise ValueError("%s: the bias is a mapping {event name or class id: float}, got %s"
                             % (where, type(events).__name__))
        row = np.zeros(n, dtype=np.float32)
        for ev, value in events.items():
            v = self._finite(value, "%s: the bias of %r" % (where, ev))
            if isinstance(ev, (int, np.integer)) and not isinstance(ev, bool):
                if not 0 <= int(ev) < n:
                    raise ValueError("%s: class id %d out of range (%d classes)" % (where, int(ev), n))
                row[int(ev)] = v
                continue
            ids = [i for i, e in names.items() if e == ev]
            if not ids:
                raise ValueError("%s: unknown event %r" % (where, ev))
            row[ids] = v
        return row

    @property
    def has_bias(self):
        return bool(self.static or self.schedule)

    @property
    def has_penalty(self):
        return bool(self.frequency.any() or self.presence.any())

    def bias_row(self, bar):
        """The (sum n_class,) f32 bias of a row drawn at bar count `bar` (the count before the row)."""
        out = []
        i = max(int(bar) - 1, 0)
        for a, n in enumerate(self.n_class):
            if a in self.static:
                out.append(self.static[a])
            elif a in self.schedule:
                sch = self.schedule[a]
                out.append(sch[i % len(sch)] if self.cycle else sch[min(i, len(sch) - 1)])
            else:
                out.append(np.zeros(n, dtype=np.float32))
        return np.concatenate(out).astype(np.float32)

    def bias_rows(self, bar_cond):
        """The device table of this preference's bias for songs that end at bar `bar_cond` -> (R, sum n_class) f32, row i
        is bar i + 1, R by the rule of Constraint.mask_rows: 1 without a schedule, bar_cond - 1 under cycle=True, else
        the longest schedule cut at bar_cond - 1.  The device clamps to the last row."""
        last = max(1, int(bar_cond) - 1)
        if not self.schedule:
            R = 1
        elif self.cycle:
            R = last
        else:
            R = min(max(len(v) for v in self.schedule.values()), last)
        return np.stack([self.bias_row(i + 1) for i in range(R)])

    def penalties(self):
        """(2 A + 1,) f32: frequency[A], presence[A], decay -- one row of the device's penalty table."""
        return np.concatenate([self.frequency, self.presence, [self.decay]]).astype(np.float32)

    def seen_states(self, song):
        """The repetition state after each row of `song` ((L, A) rows) -> (L, sum n_class) f32, from a zero state, in
        np.float32 with the product and the sum as two separate operations: what cwlt_prefer_track and cwlt_prefer_scan
        compute, bitwise.  Row L - 1 of a prompt is the seen0 its song starts from."""
        song = np.asarray(song, dtype=np.int64).reshape(-1, len(self.n_class))
        off = np.concatenate([[0], np.cumsum(self.n_class)[:-1]]).astype(np.int64)
        W = int(sum(self.n_class))
        out = np.zeros((len(song), W), dtype=np.float32)
        s = np.zeros(W, dtype=np.float32)
        inside = (song >= 0) & (song < np.asarray(self.n_class))
        for t, row in enumerate(song):
            hit = np.zeros(W, dtype=np.float32)
            hit[(off + row)[inside[t]]] = 1.0
            s = s * self.decay
            s = s + hit
            out[t] = s
        return out


def compile_preferences(preferences, n_songs, n_token, bar_cond):
    """The device tables of `preferences` (one Preference for every song, or a list of n_songs entries, None = none) ->
    None when no song has a preference, else (sched (n_songs, 2) int64 {first bias row, rows}, bias (R, sum n_class)
    f32, pen (n_songs, 2 A + 1) f32 {frequency, presence, decay}).  One Preference object's bias rows are shared by all
    songs that use it; a song without a bias has 0 rows, a song without a preference an all-zero pen row."""
    if isinstance(preferences, Preference):
        preferences = [preferences] * n_songs
    elif isinstance(preferences, (list, tuple)):
        if len(preferences) != n_songs:
            raise ValueError("preferences: %d entries for %d songs" % (len(preferences), n_songs))
    else:
        raise ValueError("preferences must be a Preference or a list of n_songs Preference / None entries, got %s"
                         % type(preferences).__name__)
    if all(p is None for p in preferences):
        return None
    W, A = int(sum(n_token)), len(n_token)
    sched = np.zeros((n_songs, 2), dtype=np.int64)
    pen = np.zeros((n_songs, 2 * A + 1), dtype=np.float32)
    parts, rows, total = [], {}, 0
    for k, p in enumerate(preferences):
        if p is None:
            continue
        if not isinstance(p, Preference):
            raise ValueError("preferences[%d] is a %s, not a Preference or None" % (k, type(p).__name__))
        if list(p.n_class) != list(n_token):
            raise ValueError("preferences[%d] was built for classes %s, the model draws %s" % (k, p.n_class,
                                                                                            list(n_token)))
        pen[k] = p.penalties()
        if not p.has_bias:
            continue
        if id(p) not in rows:
            parts.append(p.bias_rows(bar_cond))
            rows[id(p)] = (total, len(parts[-1]))
            total += len(parts[-1])
        sched[k] = rows[id(p)]
    bias = np.concatenate(parts) if parts else np.zeros((0, W), dtype=np.float32)
    return sched, np.ascontiguousarray(bias, dtype=np.float32), pen


def sampler_settings(sampler):
    """sampler -> (temperature, top_p) per attribute: "dqn" forward_output_sampling's, "categorical" the plain draw."""
    if sampler not in ("dqn", "categorical"):
        raise ValueError("sampler must be 'dqn' or 'categorical', got %r" % (sampler,))
    return (DQN_TEMPERATURE, DQN_TOP_P) if sampler == "dqn" else (None, None)


def check_entry(model, what, sampler=None, like=None, **kernel):
    """The first refusals of an entry, which `what` names in the messages: the names of its sampler and of its prefill
    kernel (given as prefill= or kernel=), then the model's state: recurrent, eval(), f32 activations.  like (for a
    reference model): the model it goes with, whose classes and device it must have."""
    if sampler is not None:
        sampler_settings(sampler)
    for name, value in kernel.items():
        if value not in ("blas", "gemm", "packed"):
            raise ValueError("%s must be 'blas' or 'gemm' (or 'packed', gemm's bits without padded rows), got %r"
                             % (name, value))
    if not getattr(model, "_recurrent", False):
        raise RuntimeError("%s needs a model built with is_training=False (recurrent encoder)" % what)
    if model.training:
        raise RuntimeError("%s runs in eval() mode (agent_pretrain.py:657)" % what)
    if model.compute_dtype != torch.float32:
        gemm = "the GEMM decode step computes in f32: this model runs %s activations (generate one song at a time " \
               "with fused=False instead)"
        raise RuntimeError((gemm if what == "generation" else what + " computes in f32: this model runs %s activations")
                           % model.compute_dtype)
    if like is not None:
        if list(model.n_token) != list(like.n_token):
            raise ValueError("the reference model has classes %s, the model %s" % (list(model.n_token),
                                                                                  list(like.n_token)))
        dev = next(like.parameters()).device
        if next(model.parameters()).device != dev:
            raise ValueError("the reference model must sit on the model's device (%s)" % (dev,))


class DrawPlan:
    """The host stage: what the sampler draws from for the `n_songs` songs of one call of entry `where` -- the refusals
    of constraints / grammar / reference / alpha, then their tables.  No device work, no seed.  Fields: n_token;
    temperature, top_p; table = compile_constraints' (sched, masks) or None, with it bar_mask ((n_class[2],) int32, 1 at
    the classes named "Bar"); gram = compile_grammar's (order, gram) with bar_attr, or None; alpha = compile_alpha's
    table or None; reference (the model) or None; logprobs; bar0s, each song's bar count before its first drawn row;
    under a grammar beat0s, its position there (after its `heads` entry; no heads: none, a scorer's rows carry theirs).
    bar_cond, bar0s, max_tokens: compile_constraints'; the scorers pass their largest bar count + 1, [1] * n and the
    longest song (a given song ends: "could never end" is no refusal).  what: "generation" or "scoring", in the
    reference's refusals.  lone_reference (policy_stats): a reference needs no alpha.
    preferences: prefer = compile_preferences' (sched, bias, pen) or None; seen0s, (n_songs, sum n_class)
    f32, each song's repetition state after its `heads` entry (Preference.seen_states; zeros without a preference), None
    when no song has a non-zero penalty or there are no heads (a scorer's rows carry theirs); bar_mask is then also set
    when some song's bias schedule has more than one row, so that a loop can count bars for it.  Without preferences
    every other field is what it was."""

    def __init__(self, model, word2event, n_songs, where, sampler="categorical", constraints=None, grammar=None,
                 reference=None, alpha=None, logprobs=False, bar_cond=None, bar0s=None, max_tokens=None, heads=None,
                 what="generation", lone_reference=False, preferences=None):
        self.n_token, self.n_songs = list(model.n_token), int(n_songs)
        self.temperature, self.top_p = sampler_settings(sampler)
        self.logprobs, self.reference = bool(logprobs), reference
        self.constraints, self.grammar, self.bar_cond, self.max_tokens = constraints, grammar, bar_cond, max_tokens
        self.bar0s = [1] * self.n_songs if bar0s is None else list(bar0s)
        self.table = self.bar_mask = self.gram = self.bar_attr = self.beat0s = self.alpha = None
        self.preferences, self.heads, self.prefer, self.seen0s = preferences, heads, None, None
        self._bar_names = None if "bar-beat" not in word2event else word2event["bar-beat"]
        if alpha is not None and reference is None:
            raise ValueError("%salpha blends the model with a reference model: pass reference= as well"
                             % ("" if lone_reference else where + ": "))
        if reference is not None:
            if alpha is None and not lone_reference:
                raise ValueError("%s: reference= needs alpha= (1: the model, 0: the reference; the reference's own "
                                 "songs or scores come from calling %s on it)" % (where, where))
            check_entry(reference, "the reference model: " + what, like=model)
        if self.n_songs == 0:
            return                                               # the scorers' empty list: nothing to compile
        if alpha is not None:
            self.alpha = compile_alpha(alpha, self.n_songs, len(self.n_token))
        self._compile_constraints()
        if self.table is not None:
            self.bar_mask = self._bar_classes()
        if grammar is not None:
            self.gram = compile_grammar(grammar, constraints, self.n_songs, self.n_token, bar_cond)
            self.bar_attr = grammar.bar_attr
            at = {}                                              # one shared prompt: one walk over it
            self.beat0s = [] if heads is None else \
                [at[id(h)] if id(h) in at else at.setdefault(id(h), grammar.beat_states(h)[1]) for h in heads]
        if preferences is not None:
            self._compile_preferences()

    def _bar_classes(self):
        names = self._bar_names
        return np.array([names[i] == "Bar" for i in range(self.n_token[2])], dtype=np.int32)

    @property
    def penalised(self):
        """True when some song has a non-zero frequency or presence penalty."""
        return self.prefer is not None and bool(self.prefer[2][:, :-1].any())

    @property
    def bias_bars(self):
        """True when some song's bias schedule has more than one row: its draw needs the song's bar count."""
        return self.prefer is not None and bool((self.prefer[0][:, 1] > 1).any())

    def _compile_preferences(self):
        """prefer and seen0s of the plan's own songs (self.preferences, self.heads), and bar_mask for a bias schedule."""
        self.prefer = compile_preferences(self.preferences, self.n_songs, self.n_token, self.bar_cond)
        self.seen0s = None
        self.bar_mask = self._bar_classes() if self.table is not None or self.bias_bars else None
        if not self.penalised or self.heads is None:
            return
        prefs = self.preferences if isinstance(self.preferences, (list, tuple)) else [self.preferences] * self.n_songs
        self.seen0s = np.zeros((self.n_songs, int(sum(self.n_token))), dtype=np.float32)
        at = {}                                                  # one shared prompt and preference: one walk
        for k, (p, h) in enumerate(zip(prefs, self.heads)):
            if p is not None and len(h):
                key = (id(p), id(h))
                if key not in at:
                    at[key] = p.seen_states(h)[-1]
                self.seen0s[k] = at[key]

    def _compile_constraints(self):
        self.table = None if self.constraints is None else compile_constraints(
            self.constraints, self.n_songs, self.n_token, self.bar_cond, self.bar0s, self.max_tokens)

    def songs(self, first, count):
        """The plan of songs [first, first + count): list constraints and preferences, per-song alpha rows, bar counts,
        positions and repetition states are cut (a cut list is compiled as the group's own call would), what every song
        shares passes through."""
        p = copy.copy(self)
        cut = slice(first, first + count)
        p.n_songs, p.bar0s = count, self.bar0s[cut]
        p.beat0s = self.beat0s and self.beat0s[cut]
        if self.alpha is not None and len(self.alpha) > 1:
            p.alpha = np.ascontiguousarray(self.alpha[cut])
        if isinstance(self.constraints, (list, tuple)):
            p.constraints = list(self.constraints[cut])
            p._compile_constraints()
        elif self.table is not None:
            p.table = (self.table[0][cut], self.table[1])
        if self.preferences is not None:
            p.heads = None if self.heads is None else list(self.heads[cut])
            if isinstance(self.preferences, (list, tuple)):
                p.preferences = list(self.preferences[cut])
            p._compile_preferences()
        return p


class DeviceDraw:
    """The device stage: a DrawPlan's tables on `dev`, uploaded once, for the token loops, _draw_token and the scorers:
    sched (n_songs, 2) int64 and masks (R, W) int32 (the mask words' view), or None; order (n_class[bar_attr],) int32,
    gram (3, W) int32, beat0 (n_songs,) int64 and bar_attr, or None; alpha (1 | n_songs, A) f32 or None; ref, the
    reference's session, or None; temperature, top_p, logprobs; the host's bar0s and bar_mask.  Under preferences
     pen (n_songs, 2 A + 1) f32, with psched (n_songs, 2) int64 and bias (R, sum n_class) f32 when some
    song has a bias (else None), seen0 (n_songs, sum n_class) f32 when some song has a penalty and the plan has heads
    (else None), and the plan's flags penalised and bias_bars.  No plan: the plain draw at temperature 1.  What moves per
    token or row (bar counts, positions, song keys, repetition states) is passed beside it."""

    temperature = top_p = sched = masks = order = gram = beat0 = bar_attr = alpha = bar0s = bar_mask = None
    pen = psched = bias = seen0 = None
    logprobs = penalised = bias_bars = False

    def __init__(self, plan=None, dev=None, ref=None):
        self.ref = ref
        if plan is None:
            return
        up = lambda x: torch.as_tensor(x).to(dev)
        words = lambda x: up(np.ascontiguousarray(x).view(np.int32))
        self.temperature, self.top_p, self.logprobs = plan.temperature, plan.top_p, plan.logprobs
        self.bar0s, self.bar_mask = plan.bar0s, plan.bar_mask
        if plan.table is not None:
            self.sched, self.masks = up(plan.table[0]), words(plan.table[1])
        if plan.gram is not None:
            self.order, self.gram, self.bar_attr = up(plan.gram[0]), words(plan.gram[1]), plan.bar_attr
            self.beat0 = up(np.asarray(plan.beat0s, dtype=np.int64))
        if plan.alpha is not None:
            self.alpha = up(plan.alpha)
        if plan.prefer is not None:
            sched, bias, pen = plan.prefer
            self.pen, self.penalised, self.bias_bars = up(pen), plan.penalised, plan.bias_bars
            if len(bias):
                self.psched, self.bias = up(sched), up(bias)
            if plan.seen0s is not None:
                self.seen0 = up(plan.seen0s)

    def keywords(self, bar=None, **key):
        """The sampler settings and, at bar counts `bar`, the constraint table: keywords of ops' samplers / scorers."""
        m = {} if self.sched is None else dict(key, bar=bar, sched=self.sched, masks=self.masks)
        return dict(m, temperature=self.temperature, top_p=self.top_p)

    def grammar(self, beat):
        """(beat, order, gram, bar_attr) at positions `beat`, None without a grammar."""
        return None if self.order is None else (beat, self.order, self.gram, self.bar_attr)
