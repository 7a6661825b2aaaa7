"""The text files CommonWriter keeps beside the particle dumps (src/writers/CommonWriter.cc).

WaveGage.txt: a header `time<TAB>zgage0<TAB>zgage1...` (:72-80) and one line per write, the time and the level of every gage at the
stream's precision of 9 significant digits (:244-252).

energy.txt: a header `time`, three columns per fluid of the problem, three for everybody else and `total` (:53-70), and one line per
write at 16 significant digits (:226-241); the total adds the problem's fluids and the non-fluid class, in that order."""
from .defs import MAX_FLUID_TYPES


def _g9(x):
    return "%.9g" % float(x)      # an ostream with precision(9) and the default float format; NaN prints as "nan" in both


def _g16(x):
    return "%.16g" % float(x)


def wave_gage_header(num_gages):
    return "time" + "".join("\tzgage%d" % g for g in range(int(num_gages))) + "\n"


def wave_gage_line(t, z):
    return _g9(t) + "".join("\t" + _g9(v) for v in z) + "\n"


def energy_header(num_fluids):
    return ("time" + "".join("\tkinetic%d\tpotential%d\tinternal%d" % (f, f, f) for f in range(int(num_fluids)))
            + "\tkineticNF\tpotentialNF\tinternalNF\ttotal\n")


def energy_total(energy, num_fluids):
    """what write_energy adds up: kinetic + potential + internal of every fluid of the problem, then of the non-fluid class"""
    total = 0.0
    for c in list(range(int(num_fluids))) + [MAX_FLUID_TYPES]:
        total += float(energy[c][0]) + float(energy[c][1]) + float(energy[c][2])
    return total


def energy_line(t, energy, num_fluids):
    """energy: [MAX_FLUID_TYPES + 1][3] (kinetic, potential, internal) per fluid, the non-fluid class last"""
    classes = list(range(int(num_fluids))) + [MAX_FLUID_TYPES]
    return (_g16(t) + "".join("\t" + _g16(energy[c][k]) for c in classes for k in range(3))
            + "\t" + _g16(energy_total(energy, num_fluids)) + "\n")
