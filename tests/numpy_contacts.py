"""Independent numpy restatement of the body rows of rr_contact_observations (include/realrobot.h): per body {max, sum} of the
normal force and a bit mask of what the body touches, from contact lists in the layout of rr_get_contacts / Kuka.get_contacts
(robot.py:131-150).  Written from the header's description alone; a sequential float32 loop in contact order, so that the
device's sums can be compared bit for bit."""
import numpy as np

N_OBJECTS = 3
CONTACT_THRESHOLD = np.float32(0.1)      # robot.py:136
BIT_STATIC, BIT_ROBOT = 1, 16            # bit 0; bit 4 (object j: bit 1 + j)


def body_rows(contact_lists, n_links=17):
    """contact_lists: one [k, 12] array per env, rows {bodyA, bodyB, linkA, x, y, z, nx, ny, nz, distance, normal_force, mu}
    (body -1 static, 0..15 a robot body, 16 + i object i).  Returns (body_force float32 [n, R, 2] = {max, sum},
    body_partners uint32 [n, R]) with R = n_links + 3: rows 0..n_links-1 the robot's links, n_links + i object i."""
    R = n_links + N_OBJECTS
    force = np.zeros((len(contact_lists), R, 2), np.float32)
    partners = np.zeros((len(contact_lists), R), np.uint32)

    def add(e, row, f, bit):
        if f > force[e, row, 0]:
            force[e, row, 0] = f
        force[e, row, 1] = np.float32(force[e, row, 1] + f)      # one float32 add after the other
        partners[e, row] |= np.uint32(bit)

    for e, rows in enumerate(contact_lists):
        for r in np.asarray(rows, np.float32).reshape(-1, 12):
            a, b, link = int(r[0]), int(r[1]), int(r[2])
            if not abs(r[9]) < CONTACT_THRESHOLD:
                continue
            f = np.float32(r[10])
            a_robot = 0 <= a < 16
            bit_of_b = BIT_STATIC if b < 0 else (2 << (b - 16) if b >= 16 else BIT_ROBOT)
            if a_robot:
                add(e, link, f, bit_of_b)
            elif a >= 16:
                add(e, n_links + a - 16, f, bit_of_b)
            if b >= 16:
                add(e, n_links + b - 16, f, BIT_ROBOT if a_robot else 2 << (a - 16))
    return force, partners
