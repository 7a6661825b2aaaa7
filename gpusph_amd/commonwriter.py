"""The text files CommonWriter keeps beside the particle dumps (src/writers/CommonWriter.cc); of them WaveGage.txt:
a header `time<TAB>zgage0<TAB>zgage1...` (:72-80) and one line per write, the time and the level of every gage at the stream's
precision of 9 significant digits (:244-252)."""


def _g9(x):
    return "%.9g" % float(x)      # an ostream with precision(9) and the default float format; NaN prints as "nan" in both


def wave_gage_header(num_gages):
    return "time" + "".join("\tzgage%d" % g for g in range(int(num_gages))) + "\n"


def wave_gage_line(t, z):
    return _g9(t) + "".join("\t" + _g9(v) for v in z) + "\n"
