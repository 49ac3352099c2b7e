"""What a spectra request becomes: which tracer a name is, whether a set of pairs fits the batched mass integrals, which
registered tracers ride along with a cached request, and the pair bookkeeping of a batch.  Plain data in, plain data
out: nothing here calls into the library or holds device state; ``HaloModel`` builds the structures and issues the calls."""
from collections import namedtuple

BATCH_NAMES = 4           # distinct tracers the batched mass integrals take


class Resolved(namedtuple("Resolved", "name kind1 kind2 tensors1 tensors2")):
    """One resolved name.  kind1 / kind2: what the 1-halo (hods, uk, pk: hmvec/hmvec.py:516-523) and the 2-halo lookup
    (uk, pk, hods: hmvec/hmvec.py:537-550) find, as "h" (HOD), "m" (matter profile) or "p" (pressure profile);
    tensors1 / tensors2: the profile tensors that tracer streams, as ((dict tag "uk" | "pk", tensor name), ...) - of an
    HOD its satellite profile and, if it has one, its central profile."""
    __slots__ = ()

    def found(self, term):
        """(kind, tensors) of the 1-halo (term 1) or 2-halo (term 2) lookup."""
        return (self.kind1, self.tensors1) if term == 1 else (self.kind2, self.tensors2)

    @property
    def same(self):
        """Do both lookups find the same tracer (one fused launch serves both terms)?"""
        return self.kind1 == self.kind2


def _tensors(name, kind, hods):
    if kind != "h":
        return (("uk" if kind == "m" else "pk", name),)
    sat, cen = hods[name]["satellite_profile"], hods[name]["central_profile"]
    return (("uk", sat),) if cen is None else (("uk", sat), ("uk", cen))


def resolve(name, hods, uk, pk):
    """The Resolved record of `name`.  hods: name -> mapping with "satellite_profile" and "central_profile" (a name or
    None); uk, pk: the names of the matter and the pressure profiles."""
    hod, matter, pressure = name in hods, name in uk, name in pk
    if not (hod or matter or pressure):
        raise ValueError(f"no HOD, matter profile or pressure profile is named {name!r}")
    kind1 = "h" if hod else "m" if matter else "p"
    kind2 = "m" if matter else "p" if pressure else "h"
    t1 = _tensors(name, kind1, hods)
    return Resolved(name, kind1, kind2, t1, t1 if kind2 == kind1 else _tensors(name, kind2, hods))


def check_term(term, terms):
    """Refuse a term of a request that is not one of `terms`."""
    if term not in terms:
        raise ValueError(f"term must be one of {terms}, got {term!r}")


def _same_lookups(recs, what):
    """Refuse a request of `what` that names something the 1-halo and 2-halo lookups resolve differently."""
    for r in recs:
        if not r.same:
            raise ValueError(f"{what}: the 1-halo and 2-halo lookups resolve {r.name!r} differently (it names both an HOD "
                             f"and a profile)")


def first_name_rule(a, b):
    """Two different HOD (or two different pressure) names: the reference uses the first name's square term
    (hmvec/hmvec.py:510-513), so the spectrum depends on the order - the batched kernel computes each unordered pair
    once, these stay on the one-pair kernel."""
    return a.name != b.name and a.kind1 == b.kind1 and a.kind1 in "hp"


def batchable(names, pairs):
    """Can the batched mass integrals express these (Resolved, Resolved) pairs with the reference's semantics?  names:
    the distinct records of the pairs."""
    return (len(names) <= BATCH_NAMES and all(t.same for t in names)
            and not any(first_name_rule(a, b) for a, b in pairs))


def with_riders(a, b, registered, valid, small):
    """The (Resolved, Resolved) pairs of the batch a cached request for (a, b) is computed in, or [] if it has to take the
    one-pair kernel.  Other registered tracers ride along - their spectra with each other and with the request are
    cached by the same pass - if their tensors are among those the request streams anyway: then they cost no HBM
    traffic.  On a small grid (`small`) a tensor more costs microseconds while a batch more costs a launch and a result
    copy, so there any registered tracer rides.  registered: the records of hods, uk_profiles, pk_profiles in that order
    (read only while the batch has room); valid(tag, tensor name): is that tensor on the device in the model's shape -
    a rider that is not (a hand-assigned entry can be anything) must not break the request it would ride with."""
    def ok(t):
        return t.same and all(valid(*tn) for tn in t.tensors1)
    if not (ok(a) and ok(b)):
        return []
    need = set(a.tensors1) | set(b.tensors1)
    batch = [a] if a.name == b.name else [a, b]
    for cand in registered:
        if all(cand.name != t.name for t in batch) and (small or set(cand.tensors1) <= need) and ok(cand):
            batch.append(cand)
            if len(batch) == BATCH_NAMES:
                break
    pairs = [(x, y) for i, x in enumerate(batch) for y in batch[i:] if not first_name_rule(x, y)]
    return pairs if (a, b) in pairs or (b, a) in pairs else []


def pair_plan(pairs):
    """The bookkeeping of a batch of (a, b) pairs, (a, b) and (b, a) being the same spectrum: (names, unique, alias,
    first) - the distinct names in first-seen order; the unique unordered pairs as sorted index pairs into names, in
    first-seen order; per requested pair the index of its unique pair; per unique pair the first request of it."""
    names, unique, alias = [], [], []
    for pair in pairs:
        for n in pair:
            if n not in names:
                names.append(n)
        key = tuple(sorted(names.index(n) for n in pair))
        if key not in unique:
            unique.append(key)
        alias.append(unique.index(key))
    return names, unique, alias, [alias.index(u) for u in range(len(unique))]
