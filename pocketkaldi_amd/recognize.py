"""The reference's command-line program (main.cc:17-80) over the Recognizer.

    python -m pocketkaldi_amd.recognize <model-file> <x.wav | x.scp> [--ctm] [--reference-softmax] [--channel N]
                                        [--frontend key=value,...] [--deltas order=N,window=N]
                                        [--cmvn mode=...,norm_means=...,norm_vars=... [--cmvn-stats RX [--utt2spk FILE]]]
                                        [--cmvn mode=online,cmn_window=...,speaker_frames=...,global_frames=...,norm_vars=...
                                         [--cmvn-global RX] [--cmvn-stats RX [--utt2spk FILE]]]
                                        [--online [--chunk-ms N] [--partials] [--commit]
                                         [--endpoint-silence 0,1,2 [--endpoint-rule must,trail_s,relcost,len_s ...]]]
    python -m pocketkaldi_amd.recognize <model-file> <feats.npy | feats.npz | x.ark | x.scp | ark:... | scp:...>
                                        --features raw|normalized [--ctm] [--reference-softmax] [--online ...]

One line per wave, main.cc:28's "%s\\t%s\\t%f\\n": the file, the sentence, the log-likelihood per frame.  An input
that does not end in .wav is a list of wave files, one per line (main.cc:34-46); its waves are decoded together, as
many per call as the recognizer holds.  --ctm prints the word times instead: "<file> 1 <start> <duration> <word>"
per word segment of the best path, in seconds at the 10 ms frame shift (fbank.cc:35-42); segments without a word
(word 0: what precedes the first word of a path) are skipped.

Every file is read with read_wave: any sample rate from 8 to 96 kHz and up to 8 channels, of which --channel N
(default 0) is taken; audio that is not at 16 kHz is converted on the GPU on the way in, and the word times stay on
the 10 ms frame grid of the converted audio.

--features KIND takes features instead of audio (Recognizer.process_features): a .npy file holds one [T][D] matrix and is
printed under the file's name, a .npz file holds one utterance per array and each is printed under its array's name, in
the file's order.  A Kaldi archive or script file of matrices (x.ark, x.scp, ark:<path>, scp:<path>; pk.ArkReader) holds
one utterance per entry, printed under its key; its entries are read and decoded in groups of at most MAX_UTTS utterances
and MAX_SAMPLES / 160 frames, not all read first.  KIND raw: 40-dim log-mel fbank, the CMVN is applied; normalized: ready
for the splice.  --ctm works as it does for audio.  With --online every utterance goes through
OnlineRecognizer.open_features / push_features, max(1, chunk-ms // 10) frames per step, and --partials, --commit,
--endpoint-silence and --endpoint-rule work as they do for audio, at 10 ms per frame; stdout is what it is without
--online, and what --online prints for the audio the features came from.

--frontend key=value,... takes a model of another front-end than the reference's (pk.FrontendSpec),
for example kind=mfcc,num_mel_bins=23,num_ceps=13,window=povey,low_freq=20,high_freq=-400,cepstral_lifter=22.  The keys
are FrontendSpec's field names, omitted keys take its defaults; an unknown key or a value that does not parse is refused
with the key named and the usage text.  The model file's cmvn_stats then has the spec's dimension + 1 entries, and
--features matrices are [T][dimension].  It combines with every other flag; without it nothing changes.

--cmvn mode=sliding|none|utterance|speaker,norm_means=true|false,norm_vars=true|false takes a model that was trained with
Kaldi's apply-cmvn instead of the sliding rule (pk.NormSpec): per utterance, per speaker, with or
without variance, or not at all.  It works with every batch form -- wave files and lists, --features raw matrices and
archives, --frontend.  Mode speaker needs --cmvn-stats RX, an archive or script file of 2 x (D + 1) statistics matrices
(compute-cmvn-stats' output; ark:<path>, scp:<path> or a path), keyed by what this program prints in front of an
utterance's line -- or by speaker, with --utt2spk FILE ("<utterance> <speaker>" per line).  An utterance or a speaker
without an entry is refused with its name and the usage text, as are --cmvn-stats without mode=speaker and mode=speaker
without --cmvn-stats.  With --features normalized the matrices are ready for the splice and no norm applies.  With
--online the modes none, speaker and online (below) run on the online objects and print what the batch form prints;
mode=utterance with --online is refused with the usage text: an utterance's statistics do not exist while it is live.

--cmvn mode=online,cmn_window=600,speaker_frames=600,global_frames=200,norm_vars=true|false takes a model that was trained
on apply-cmvn-online's features (pk.OnlineCmvnSpec): Kaldi's online CMVN over every whole
utterance, on the batch scorer or, with --online, live.  --cmvn-global RX names the 2 x (D + 1) global statistics (pk.kaldi_cmvn_stats) the window
is smoothed with; global_frames > 0 without it is refused with the usage text.  --cmvn-stats and --utt2spk give the
speakers' statistics as for mode=speaker; here they are optional.

--deltas order=2,window=2 takes a model that was trained on add-deltas' features (pk.DeltaSpec): its
first layer expects (order + 1) x the dimension of the front-end -- the reference's, or --frontend's -- and the model
file's cmvn_stats, --cmvn-stats and --cmvn-global are at the front-end's dimension: the deltas are taken behind the
normalisation.  It works with every batch form -- wave files and lists, --features raw matrices and archives ([T][front-end's
dimension]), --frontend, --cmvn.  --features normalized --deltas takes matrices that are ready for the splice,
[T][(order + 1) x the front-end's dimension], and no deltas are added.  With --online it is refused with the usage text:
the live objects do not have deltas yet.

--transform matrix=final.mat,left_context=3,right_context=3 takes a model that was trained on splice-feats |
transform-feats features (LDA+MLLT; pk.TransformSpec): the matrix (a Kaldi matrix file) is applied
behind the normalisation and the deltas, and the model file's cmvn_stats, --cmvn-stats and --cmvn-global are at the
front-end's dimension.  --utt-transforms ark:trans.ark names a Kaldi archive of per-utterance matrices (fMLLR), applied
behind the global one (or alone), keyed by utterance or, with --utt2spk FILE, by speaker; a missing key is refused with
the usage text and named.  Both work with every batch form and with --frontend, --cmvn and --deltas; --features
normalized matrices are past every stage and take neither.  With --online either is refused with the usage text: the
live objects do not have transforms yet.

--online feeds the waves as live audio through the OnlineRecognizer, --chunk-ms N (default 100) milliseconds per step
(measured at the file's own rate),
up to MAX_UTTS waves at a time, a slot each; what it prints on stdout is what it prints without the flag.  --partials
also prints every changed partial hypothesis to stderr: "<file>\t<seconds of audio fed>\t<text>".  --chunk-ms and
--partials without --online are refused with the usage text, as is --commit.  --commit turns the online decoder's commit
mode on (streams of any length; pk_mi355_online_decoder_set_commit): stdout is unchanged, and every --partials line gains
a fourth tab field, the stable text -- the words of the partial that no later audio can change.

--endpoint-silence P,Q,... (with --online) turns endpointing on with these pdfs as silence: a wave is cut into utterances
where an endpoint rule fires, and stdout has one line per utterance, "<file>[<start s>-<end s>]\t<sentence>\t<llpf>";
with --ctm the word times are offset by the utterance's start.  The rules are the usual five unless --endpoint-rule gives
others, one "must_contain_nonsilence,min_trailing_silence_s,max_relative_cost,min_utterance_length_s" each (inf allowed).
"""
import sys

import pocketkaldi_amd as pk

FRAME_SHIFT = 0.01
MAX_UTTS = 16
MAX_SAMPLES = 16000 * 120
RESERVE = 32


def usage():
    print("Usage: python -m pocketkaldi_amd.recognize <model-file> <input-file> [--ctm] [--reference-softmax] [--channel N] "
          "[--frontend key=value,...] [--deltas order=N,window=N] [--transform matrix=FILE,left_context=N,right_context=N] "
          "[--utt-transforms RX [--utt2spk FILE]] [--cmvn mode=...,norm_means=...,norm_vars=... [--cmvn-stats RX [--utt2spk FILE]]] "
          "[--cmvn mode=online,cmn_window=...,speaker_frames=...,global_frames=...,norm_vars=... [--cmvn-global RX] [--cmvn-stats RX [--utt2spk FILE]]] "
          "[--online [--chunk-ms N] [--partials] [--commit] [--endpoint-silence P,Q,... [--endpoint-rule M,T,C,L ...]]]")
    print("       python -m pocketkaldi_amd.recognize <model-file> <feats.npy | feats.npz | x.ark | x.scp | ark:... | scp:...> "
          "--features raw|normalized [--ctm] [--reference-softmax] [--cmvn ...] [--deltas ...] [--transform ...] [--utt-transforms ...] [--online ...]")
    print("  --deltas order=N,window=N: add-deltas behind the normalisation (not with --online); --features raw matrices are [T][front-end's "
          "dimension], --features normalized matrices [T][the model's dimension] and take no deltas.")
    print("  --transform matrix=FILE,left_context=N,right_context=N[,in_dim=N]: splice-feats | transform-feats behind the normalisation and "
          "the deltas (not with --online); --utt-transforms RX: a Kaldi archive of per-utterance matrices applied behind it, keyed by utterance, "
          "or by speaker with --utt2spk.")
    print("  Input-file:")
    print("    *.wav: decode this file.")
    print("    *.scp: decode audios listed in it.")
    print("    *.npy / *.npz (with --features): decode this feature matrix / every array of the file.")
    print("    *.ark / *.scp / ark:<path> / scp:<path> (with --features): decode every matrix of this Kaldi archive / script file.")
    return 1


class Norm:
    """--cmvn and what goes with it: the spec, and for mode speaker the statistics by key and the utterance-to-speaker map."""

    def __init__(self, spec, stats=None, utt2spk=None, global_stats=None):
        self.spec, self.stats, self.utt2spk, self.global_stats = spec, stats, utt2spk, global_stats

    def apply(self, rec):
        if isinstance(self.spec, pk.OnlineCmvnSpec):
            rec.batch.set_norm(self.spec, self.global_stats)
        else:
            rec.batch.set_norm(self.spec)

    def apply_online(self, rec):
        """The same spec on an OnlineRecognizer's scorer."""
        if isinstance(self.spec, pk.OnlineCmvnSpec):
            rec.scorer.set_norm(self.spec, self.global_stats)
        else:
            rec.scorer.set_norm(self.spec)

    def speaker_stats(self, names):
        """The records of these utterances, or None when the mode takes none.  UsageError names a missing key."""
        if self.stats is None:
            return None
        out = []
        for name in names:
            key = name
            if self.utt2spk is not None:
                if name not in self.utt2spk:
                    raise UsageError("--utt2spk: no speaker for utterance '%s'" % name)
                key = self.utt2spk[name]
            if key not in self.stats:
                raise UsageError("--cmvn-stats: no statistics for %s '%s'" % ("speaker" if self.utt2spk is not None else "utterance", key))
            out.append(self.stats[key])
        return out


class UsageError(Exception):
    pass


def take_value(argv, flag):
    """Remove `flag VALUE` from argv -> VALUE, or None when the flag is absent.  UsageError when the value is missing."""
    if flag not in argv:
        return None
    at = argv.index(flag)
    if at + 1 >= len(argv):
        raise UsageError("%s needs a value" % flag)
    value = argv[at + 1]
    del argv[at:at + 2]
    return value


def parse_norm_flags(argv):
    """--cmvn, --cmvn-global, --cmvn-stats and --utt2spk out of argv -> a Norm, or None without --cmvn.  UsageError says
    what is wrong."""
    text, stats_rx, utt2spk_file = take_value(argv, "--cmvn"), take_value(argv, "--cmvn-stats"), take_value(argv, "--utt2spk")
    global_rx = take_value(argv, "--cmvn-global")
    if text is None:
        if stats_rx is not None or utt2spk_file is not None:
            raise UsageError("--cmvn-stats and --utt2spk go with --cmvn mode=speaker or mode=online")
        if global_rx is not None:
            raise UsageError("--cmvn-global goes with --cmvn mode=online")
        return None
    try:
        spec = pk.parse_norm(text)
        online_cmvn = isinstance(spec, pk.OnlineCmvnSpec)
        if "--online" in argv and not online_cmvn and spec.mode == pk.NORM_MODES["utterance"]:
            raise UsageError("--cmvn mode=utterance: the online objects do not take a norm spec yet that needs an utterance's statistics: "
                             "they do not exist while the utterance is live; use mode=speaker or mode=online, or leave out --online")
        if not online_cmvn:
            spec.check()
        elif spec.global_frames <= 0 or global_rx is not None:      # (global_frames > 0 without --cmvn-global: said below)
            spec.check(None, 1) if spec.global_frames <= 0 else pk.OnlineCmvnSpec(spec.cmn_window, spec.speaker_frames, 0, spec.norm_vars).check(None, 1)
    except (ValueError, pk.PkError) as e:
        raise UsageError("--cmvn: %s" % e)
    if not online_cmvn and global_rx is not None:
        raise UsageError("--cmvn-global goes with --cmvn mode=online")
    if online_cmvn and spec.global_frames > 0 and global_rx is None:
        raise UsageError("--cmvn mode=online with global_frames > 0 needs --cmvn-global (the global statistics), or global_frames=0")
    speaker = not online_cmvn and spec.mode == pk.NORM_MODES["speaker"]
    if speaker and stats_rx is None:
        raise UsageError("--cmvn mode=speaker needs --cmvn-stats")
    if not speaker and not online_cmvn and (stats_rx is not None or utt2spk_file is not None):
        raise UsageError("--cmvn-stats and --utt2spk go with --cmvn mode=speaker or mode=online")
    if online_cmvn and utt2spk_file is not None and stats_rx is None:
        raise UsageError("--utt2spk goes with --cmvn-stats")
    stats = utt2spk = global_stats = None
    if online_cmvn and global_rx is not None:
        global_stats = pk.kaldi_cmvn_stats(global_rx)
    if speaker or stats_rx is not None:
        stats = pk.read_cmvn_stats_archive(stats_rx)
        if utt2spk_file is not None:
            utt2spk = read_utt2spk(utt2spk_file)
    return Norm(spec, stats, utt2spk, global_stats)


def read_utt2spk(utt2spk_file):
    utt2spk = {}
    with open(utt2spk_file) as f:
        for n, line in enumerate(f):
            if line.strip():
                parts = line.split()
                if len(parts) != 2:
                    raise UsageError("--utt2spk: line %d of %s is not '<utterance> <speaker>'" % (n + 1, utt2spk_file))
                utt2spk[parts[0]] = parts[1]
    return utt2spk


class Transforms:
    """--transform and --utt-transforms: the spec, and the per-utterance matrices by key with the utterance-to-speaker map."""

    def __init__(self, spec, mats=None, utt2spk=None):
        self.spec, self.mats, self.utt2spk = spec, mats, utt2spk

    def utt_transforms(self, names):
        """The matrices of these utterances, or None without --utt-transforms.  UsageError names a missing key."""
        if self.mats is None:
            return None
        out = []
        for name in names:
            key = name
            if self.utt2spk is not None:
                if name not in self.utt2spk:
                    raise UsageError("--utt2spk: no speaker for utterance '%s'" % name)
                key = self.utt2spk[name]
            if key not in self.mats:
                raise UsageError("--utt-transforms: no transform for %s '%s'" % ("speaker" if self.utt2spk is not None else "utterance", key))
            out.append(self.mats[key])
        return out


def parse_transform_flags(argv):
    """--transform and --utt-transforms out of argv (and --utt2spk, unless --cmvn-stats shares it) -> a Transforms, or None
    without either.  UsageError says what is wrong."""
    text, rx = take_value(argv, "--transform"), take_value(argv, "--utt-transforms")
    if text is None and rx is None:
        return None
    if "--online" in argv:
        raise UsageError("the live objects do not have transforms yet: leave out --online")
    spec = mats = utt2spk = None
    if text is not None:
        try:
            spec = pk.parse_transform(text)
            spec.check()
        except (ValueError, pk.PkError, OSError) as e:
            raise UsageError("--transform: %s" % e)
    if rx is not None:
        try:
            mats = dict(pk.ArkReader(rx))
        except (pk.PkError, OSError) as e:
            raise UsageError("--utt-transforms: %s" % e)
        if not mats:
            raise UsageError("--utt-transforms: %s holds no matrix" % rx)
        if "--utt2spk" in argv:
            at = argv.index("--utt2spk")
            if at + 1 >= len(argv):
                raise UsageError("--utt2spk needs a value")
            utt2spk = read_utt2spk(argv[at + 1])
            if "--cmvn-stats" not in argv:               # (else the statistics are keyed by speaker too: --cmvn's parser takes the flag)
                del argv[at:at + 2]
        if spec is None:                                 # per-utterance matrices alone: no global stage, at the matrices' own dimension
            spec = pk.TransformSpec(None, in_dim=int(next(iter(mats.values())).shape[0]))
    return Transforms(spec, mats, utt2spk)


def recognize_online(model_file, files, waves, chunk_ms, reference_softmax, partials, commit=False, rates=None, endpoint=None,
                     pieces=None, frontend=None, norm=None):
    """Every wave through a slot of an OnlineRecognizer, `chunk_ms` milliseconds per step, MAX_UTTS waves at a time.
    endpoint: (silence pdfs, rules or None) turns endpointing on; pieces[u] is then wave u's list of Utterance.
    -> (the results in order, the symbol names by word id)"""
    rates = rates or [16000] * len(waves)
    # a step's capacity counts 16 kHz samples; a converted slot also counts the few a close would add (RESERVE)
    reserve = RESERVE if any(r != 16000 for r in rates) else 0
    rec = pk.OnlineRecognizer(model_file, max_streams=min(max(len(waves), 1), MAX_UTTS),
                              max_step_samples=(16 * chunk_ms + reserve) * min(max(len(waves), 1), MAX_UTTS), frontend=frontend)
    try:
        if commit:
            rec.decoder.set_commit(True)
        if endpoint:
            rec.set_endpointing(*endpoint)
        if norm:
            norm.apply_online(rec)
        return stream_waves(rec, files, waves, chunk_ms, reference_softmax, partials, commit, rates, pieces, norm=norm)
    finally:
        rec.destroy()


def stream_waves(rec, files, waves, chunk_ms, reference_softmax, partials, commit=False, rates=None, pieces=None, feature_kind=None,
                 norm=None):
    """feature_kind ("raw" / "normalized"): `waves` are [T][D] feature matrices, fed max(1, chunk_ms // 10) frames a step
    through open_features / push_features; a frame is 10 ms.  norm: the Norm whose speaker statistics the slots are opened with."""
    spk = norm.speaker_stats(files) if norm and feature_kind != "normalized" else None
    rates = [100] * len(waves) if feature_kind else rates or [16000] * len(waves)       # (units per second: frames, or samples)
    if reference_softmax:
        rec.am.set_softmax("reference")
    results = [None] * len(waves)
    for first in range(0, len(waves), MAX_UTTS):
        group = list(range(first, min(first + MAX_UTTS, len(waves))))
        pos, shown = {u: 0 for u in group}, {u: ("", "") if commit else "" for u in group}
        for u in group:
            record = spk[u] if spk else None
            rec.open_features(u - first, feature_kind, record) if feature_kind else rec.open(u - first, rates[u], record)
        live = set(group)
        while live:
            closing = []
            for u in sorted(live):
                chunk = max(rates[u] * chunk_ms // 1000, 1)
                (rec.push_features if feature_kind else rec.push)(u - first, waves[u][pos[u]:pos[u] + chunk])
                pos[u] += chunk
                if pos[u] >= len(waves[u]):          # the last chunk and the close in the same step
                    rec.close(u - first)
                    closing.append(u)
            rec.step()
            for u in sorted(live):
                text = rec.partial(u - first)
                if commit:
                    text = (text, rec.stable(u - first))
                if partials and text != shown[u]:
                    sys.stderr.write("%s\t%.2f\t%s\n" % (files[u], min(pos[u], len(waves[u])) / float(rates[u]),
                                                        "\t".join(text) if commit else text))
                    shown[u] = text
            for u in closing:
                results[u] = rec.result(u - first)
                if pieces is not None:
                    pieces[u] = rec.utterances(u - first)
                live.discard(u)
    every = results + [p.result for u in (pieces or {}) for p in pieces[u]]
    names = {s.word: rec.symbols[s.word] for r in every for s in r.segments if s.word != 0}
    return results, names


def main(argv):
    argv = list(argv)
    chunk_ms = 100
    if "--chunk-ms" in argv:
        at = argv.index("--chunk-ms")
        try:
            chunk_ms = int(argv[at + 1])
        except (IndexError, ValueError):
            return usage()
        if chunk_ms <= 0 or "--online" not in argv:
            return usage()
        del argv[at:at + 2]
    channel = 0
    if "--channel" in argv:
        at = argv.index("--channel")
        try:
            channel = int(argv[at + 1])
        except (IndexError, ValueError):
            return usage()
        if channel < 0:
            return usage()
        del argv[at:at + 2]
    features = None
    if "--features" in argv:
        at = argv.index("--features")
        if at + 1 >= len(argv) or argv[at + 1] not in pk.FEATURE_KINDS:
            return usage()
        features = argv[at + 1]
        del argv[at:at + 2]
    frontend = None
    if "--frontend" in argv:
        at = argv.index("--frontend")
        try:
            frontend = pk.parse_frontend(argv[at + 1])
        except IndexError:
            return usage()
        except ValueError as e:
            print("pocketkaldi: --frontend: %s" % e)
            return usage()
        del argv[at:at + 2]
    deltas = None
    try:
        text = take_value(argv, "--deltas")
        if text is not None:
            deltas = pk.parse_deltas(text)
            deltas.check()
            if "--online" in argv:
                raise UsageError("the live objects do not have deltas yet: leave out --online")
    except (UsageError, ValueError, pk.PkError) as e:
        print("pocketkaldi: --deltas: %s" % e)
        return usage()
    try:
        xform = parse_transform_flags(argv)
    except UsageError as e:
        print("pocketkaldi: %s" % e)
        return usage()
    try:
        norm = parse_norm_flags(argv)
    except UsageError as e:
        print("pocketkaldi: %s" % e)
        return usage()
    except (pk.PkError, OSError) as e:
        print("pocketkaldi: %s" % e)
        return 1
    endpoint, rules = None, []
    try:
        while "--endpoint-rule" in argv:
            at = argv.index("--endpoint-rule")
            must, trail, cost, length = argv[at + 1].split(",")
            rules.append(pk.EndpointRule(int(must) != 0, float(trail), float(cost), float(length)))
            del argv[at:at + 2]
        if "--endpoint-silence" in argv:
            at = argv.index("--endpoint-silence")
            endpoint = ([int(p) for p in argv[at + 1].split(",") if p], rules or None)
            del argv[at:at + 2]
    except (IndexError, ValueError):
        return usage()
    if (endpoint or rules) and (endpoint is None or "--online" not in argv):
        return usage()
    flags = [a for a in argv if a.startswith("--")]
    args = [a for a in argv if not a.startswith("--")]
    if len(args) != 2 or len(args[1]) < 4 or set(flags) - {"--ctm", "--reference-softmax", "--online", "--partials", "--commit"}:
        return usage()
    if ("--partials" in flags or "--commit" in flags) and "--online" not in flags:
        return usage()
    model_file, input_file = args
    if features and not is_feature_input(input_file):
        return usage()
    try:
        if features:
            return recognize_features(model_file, input_file, features, flags, chunk_ms, endpoint, frontend, norm, deltas, xform)
        if input_file.endswith(".wav"):
            files = [input_file]
        else:
            with open(input_file) as f:
                files = [line.strip() for line in f if line.strip()]
        waves, rates, rec, pieces = [], [], None, {}
        for name in files:
            wave, rate = pk.read_wave(name, channel)
            waves.append(wave)
            rates.append(rate)
        if "--online" in flags:
            results, names = recognize_online(model_file, files, waves, chunk_ms, "--reference-softmax" in flags,
                                              "--partials" in flags, "--commit" in flags, rates, endpoint,
                                              pieces if endpoint else None, frontend, norm)
        else:
            sizes = [pk.resample_num_output(r, len(w)) for w, r in zip(waves, rates)]       # capacity counts 16 kHz samples
            rec = pk.Recognizer(model_file, max_utts=min(max(len(waves), 1), MAX_UTTS),
                                max_total_samples=max(max(sizes + [1]), min(sum(sizes), MAX_SAMPLES)), frontend=frontend, deltas=deltas,
                                transform=xform.spec if xform else None)
            if "--reference-softmax" in flags:
                rec.am.set_softmax("reference")
            if norm:
                norm.apply(rec)
            native = any(r != 16000 for r in rates)
            results, names = rec.process(waves, rates if native else None, norm.speaker_stats(files) if norm else None,
                                         xform.utt_transforms(files) if xform else None), rec.symbols
    except UsageError as e:
        print("pocketkaldi: %s" % e)
        return usage()
    except (pk.PkError, OSError, ValueError) as e:
        print("pocketkaldi: %s" % e)                     # main.cc:10-15
        if "--online" in flags and pk.ONLINE_TIME_SPLICE_REFUSAL in str(e):
            return usage()                               # (the model file says so only once it is loaded: leave out --online)
        return 1
    emit(files, results, names, "--ctm" in flags, pieces if endpoint else None)
    if rec is not None:
        rec.close()
    return 0


def emit(files, results, names, ctm, pieces=None):
    """The output lines.  pieces (endpointing): one line per utterance, word times from the wave's start."""
    for u, name in enumerate(files if pieces is not None else []):
        for p in pieces[u]:
            if ctm:
                for s in p.result.segments:
                    if s.word != 0:
                        print("%s 1 %.2f %.2f %s" % (name, (p.first_frame + s.start_frame) * FRAME_SHIFT,
                                                     s.num_frames * FRAME_SHIFT, names[s.word]))
            else:
                sys.stdout.write("%s[%.2f-%.2f]\t%s\t%f\n" % (name, p.first_frame * FRAME_SHIFT,
                                                               (p.first_frame + p.num_frames) * FRAME_SHIFT, p.result.text,
                                                               p.result.loglikelihood_per_frame))
    for name, r in zip([] if pieces is not None else files, results):
        if ctm:
            for s in r.segments:
                if s.word != 0:
                    print("%s 1 %.2f %.2f %s" % (name, s.start_frame * FRAME_SHIFT, s.num_frames * FRAME_SHIFT, names[s.word]))
        else:
            sys.stdout.write("%s\t%s\t%f\n" % (name, r.text, r.loglikelihood_per_frame))


def is_feature_input(name):
    return name.endswith((".npy", ".npz", ".ark", ".scp")) or name.startswith(("ark:", "scp:", "ark,", "scp,"))


def feature_groups(input_file):
    """The utterances of a feature input as lists of (name, [T][D] matrix): a .npy / .npz file whole; a Kaldi archive or
    script file entry by entry, in groups of at most MAX_UTTS utterances and MAX_SAMPLES / 160 frames (an entry
    longer than that alone) -- they are not all read first."""
    import numpy as np
    if input_file.endswith(".npy"):
        yield [(input_file, np.load(input_file, allow_pickle=False))]
    elif input_file.endswith(".npz"):
        with np.load(input_file, allow_pickle=False) as z:
            yield [(k, z[k]) for k in z.files]
    else:
        group, frames = [], 0
        for key, m in pk.ArkReader(input_file):
            if group and (len(group) == MAX_UTTS or frames + m.shape[0] > MAX_SAMPLES // 160):
                yield group
                group, frames = [], 0
            group.append((key, m))
            frames += m.shape[0]
        if group:
            yield group


def recognize_features(model_file, input_file, kind, flags, chunk_ms, endpoint, frontend=None, norm=None, deltas=None, xform=None):
    """--features: every group of utterances through a Recognizer (process_features) or, with --online, through the
    slots of an OnlineRecognizer; the object is kept from group to group while the group fits it.  Raises what main
    reports; -> the exit code."""
    online = "--online" in flags
    rec, held = None, (0, 0)                             # the object, and (utterances, frames) it was made for
    step = max(chunk_ms // 10, 1)                        # frames per push
    try:
        for group in feature_groups(input_file):
            files, feats = [k for k, _ in group], [m for _, m in group]
            frames = [int(f.shape[0]) if getattr(f, "ndim", 0) == 2 else 1 for f in feats]     # (process_features names a bad shape)
            need = (min(max(len(feats), 1), MAX_UTTS), max(max(frames + [1]), min(sum(frames), MAX_SAMPLES // 160)))
            # (an online object's capacity is its streams and the step size: the frames of a group do not count)
            if rec is None or need[0] > held[0] or (not online and need[1] > held[1]):
                if rec is not None:
                    rec.destroy() if online else rec.close()
                if online:                               # (a pushed frame counts 160 samples against the step capacity)
                    rec = pk.OnlineRecognizer(model_file, max_streams=need[0], max_step_samples=160 * step * need[0], frontend=frontend)
                    if "--commit" in flags:
                        rec.decoder.set_commit(True)
                    if endpoint:
                        rec.set_endpointing(*endpoint)
                    if norm:
                        norm.apply_online(rec)
                else:
                    rec = pk.Recognizer(model_file, max_utts=need[0], max_total_samples=160 * need[1], frontend=frontend, deltas=deltas,
                                        transform=xform.spec if xform else None)
                    if "--reference-softmax" in flags:
                        rec.am.set_softmax("reference")
                    if norm:
                        norm.apply(rec)
                held = need
            pieces = {} if endpoint else None
            if online:
                results, names = stream_waves(rec, files, feats, chunk_ms, "--reference-softmax" in flags, "--partials" in flags,
                                              "--commit" in flags, None, pieces, feature_kind=kind, norm=norm)
            else:
                spk = norm.speaker_stats(files) if norm and kind == "raw" else None
                mats = xform.utt_transforms(files) if xform and kind == "raw" else None
                results, names = rec.process_features(feats, kind, spk, mats), rec.symbols
            emit(files, results, names, "--ctm" in flags, pieces)
    finally:
        if rec is not None:
            rec.destroy() if online else rec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
