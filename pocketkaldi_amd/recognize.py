"""The reference's command-line program (main.cc:17-80) over the Recognizer.

    python -m pocketkaldi_amd.recognize <model-file> <x.wav | x.scp> [--ctm] [--reference-softmax]

One line per wave, main.cc:28's "%s\\t%s\\t%f\\n": the file, the sentence, the log-likelihood per frame.  An input
that does not end in .wav is a list of wave files, one per line (main.cc:34-46); its waves are decoded together, as
many per call as the recognizer holds.  --ctm prints the word times instead: "<file> 1 <start> <duration> <word>"
per word segment of the best path, in seconds at the 10 ms frame shift (fbank.cc:35-42); segments without a word
(word 0: what precedes the first word of a path) are skipped.
"""
import sys

import pocketkaldi_amd as pk

FRAME_SHIFT = 0.01
MAX_UTTS = 16
MAX_SAMPLES = 16000 * 120


def usage():
    print("Usage: python -m pocketkaldi_amd.recognize <model-file> <input-file> [--ctm] [--reference-softmax]")
    print("  Input-file:")
    print("    *.wav: decode this file.")
    print("    *.scp: decode audios listed in it.")
    return 1


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    args = [a for a in argv if not a.startswith("--")]
    if len(args) != 2 or len(args[1]) < 4 or set(flags) - {"--ctm", "--reference-softmax"}:
        return usage()
    model_file, input_file = args
    try:
        if input_file.endswith(".wav"):
            files = [input_file]
        else:
            with open(input_file) as f:
                files = [line.strip() for line in f if line.strip()]
        waves = [pk.read_wav(name) for name in files]
        longest = max([len(w) for w in waves] + [1])
        rec = pk.Recognizer(model_file, max_utts=min(max(len(waves), 1), MAX_UTTS),
                            max_total_samples=max(longest, min(sum(len(w) for w in waves), MAX_SAMPLES)))
        if "--reference-softmax" in flags:
            rec.am.set_softmax("reference")
        results = rec.process(waves)
    except (pk.PkError, OSError) as e:
        print("pocketkaldi: %s" % e)                     # main.cc:10-15
        return 1
    for name, r in zip(files, results):
        if "--ctm" in flags:
            for s in r.segments:
                if s.word != 0:
                    print("%s 1 %.2f %.2f %s" % (name, s.start_frame * FRAME_SHIFT, s.num_frames * FRAME_SHIFT, rec.symbols[s.word]))
        else:
            sys.stdout.write("%s\t%s\t%f\n" % (name, r.text, r.loglikelihood_per_frame))
    rec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
